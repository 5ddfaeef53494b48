// Host check of the collate part of 2s-agcn_amd/csrc/sgn_plan.h (no HIP): the domain, the guarded sample selection and
// the rotation.  With two file names as its arguments it reads angles (n, 3) fp32 from the first and writes
// sgn_rotation's matrices (n, 9) fp32 to the second, for the comparison with the reference's matrices in
// tests/test_sgn_collate_cpu.py.
#include <stdio.h>
#include <vector>

#include "sgn_plan.h"

static long cases = 0, failures = 0;
#define CHECK(cond)                                                                  \
  do {                                                                               \
    ++cases;                                                                         \
    if (!(cond)) {                                                                   \
      if (++failures <= 20) printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
    }                                                                                \
  } while (0)

int main(int argc, char** argv) {
  // the domain: the sampler's, on a pool of at least one sample
  CHECK(sgn_collate_domain(1, 1, 1, 2, 2, 1, 1));
  CHECK(sgn_collate_domain(40000, 64, 300, 25, 2, 5, 20));
  CHECK(sgn_collate_domain(7, 3, SGN_SAMPLE_MAX_T, 2, 2, 1, 20));
  CHECK(!sgn_collate_domain(0, 1, 300, 25, 2, 1, 20));
  CHECK(!sgn_collate_domain(-1, 1, 300, 25, 2, 1, 20));
  CHECK(!sgn_collate_domain(7, 0, 300, 25, 2, 1, 20));
  CHECK(!sgn_collate_domain(7, 3, SGN_SAMPLE_MAX_T + 1, 25, 2, 1, 20));
  CHECK(!sgn_collate_domain(7, 3, 300, 33, 2, 1, 20));
  CHECK(!sgn_collate_domain(7, 3, 300, 25, 1, 1, 20));
  CHECK(!sgn_collate_domain(7, 3, 300, 25, 2, 0, 20));
  CHECK(!sgn_collate_domain(7, 3, 300, 25, 2, 1, 0));

  // the selection: an index outside [0, P) selects nothing
  const long long index[] = {3, 0, 6, -1, 7, 3, (long long)1 << 40, -((long long)1 << 40)};
  const long want[] = {3, 0, 6, -1, -1, 3, -1, -1};
  for (int n = 0; n < 8; ++n) CHECK(sgn_collate_source(index, n, 7) == want[n]);
  for (int n = 0; n < 7; ++n) CHECK(sgn_collate_source(nullptr, n, 7) == n);
  CHECK(sgn_collate_source(nullptr, 7, 7) == -1);

  // the rotation: identity at zero, the reference's signs on one axis at a time, orthonormal everywhere
  {
    const float zero[3] = {0.f, 0.f, 0.f};
    float R[9];
    sgn_rotation(zero, R);
    for (int i = 0; i < 9; ++i) CHECK(R[i] == (i % 4 == 0 ? 1.f : 0.f));
    const float a = 0.4f, c = cosf(a), s = sinf(a);
    const float ax[3] = {a, 0.f, 0.f}, ay[3] = {0.f, a, 0.f}, az[3] = {0.f, 0.f, a};
    sgn_rotation(ax, R);
    CHECK(R[0] == 1.f && R[4] == c && R[5] == s && R[7] == -s && R[8] == c);
    sgn_rotation(ay, R);
    CHECK(R[4] == 1.f && R[0] == c && R[2] == -s && R[6] == s && R[8] == c);
    sgn_rotation(az, R);
    CHECK(R[8] == 1.f && R[0] == c && R[1] == s && R[3] == -s && R[4] == c);
    for (int i = 0; i < 200; ++i) {
      const float ang[3] = {0.5f * sinf(1.7f * i), 0.5f * sinf(2.3f * i + 1.f), 0.5f * sinf(3.1f * i + 2.f)};
      sgn_rotation(ang, R);
      for (int p = 0; p < 3; ++p)
        for (int q = 0; q < 3; ++q) {
          const float dot = R[p * 3] * R[q * 3] + R[p * 3 + 1] * R[q * 3 + 1] + R[p * 3 + 2] * R[q * 3 + 2];
          CHECK(fabsf(dot - (p == q ? 1.f : 0.f)) < 1e-6f);
        }
      // sgn_rotate is the product with a row
      CHECK(sgn_rotate(R, 1, 1.f, 0.f, 0.f) == R[3] && sgn_rotate(R, 2, 0.f, 0.f, 1.f) == R[8]);
    }
  }
  CHECK(sgn_subject_index(2, 1, 3, 5, 20) == (2 * 5 + 1) * 20 + 3);

  if (argc > 2) {
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<float> ang;
    float a[3];
    while (fread(a, sizeof(float), 3, f) == 3) ang.insert(ang.end(), a, a + 3);
    fclose(f);
    std::vector<float> out(ang.size() * 3);
    for (size_t n = 0; n < ang.size() / 3; ++n) sgn_rotation(ang.data() + n * 3, out.data() + n * 9);
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(out.data(), sizeof(float), out.size(), f);
    fclose(f);
  }
  printf("%ld checks, %ld failures\n", cases, failures);
  return failures ? 1 : 0;
}
