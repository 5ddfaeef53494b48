"""SHA-256 digests of the SGN kernels' outputs on fixed seeds, one line per tensor, so that the logs of two builds can be
compared with `diff`: the first line that differs names the first tensor whose bits differ.

    python tools/sgn_checksums.py > sgn_checksums_<tag>.txt

Per model case: the forward (feat, g, logits), the input backward without and with the tapes (dfeat, dx), both tapes, and
the image gradients d_wf / d_wc at rows_per_split 0 and 7.  Per sampler case: out, L and the adjoint's dwin.  The model
cases are the shapes of tests/golden/sgn_paramgrad_* plus V = 32, seg = 65 (full joint rows, three clip tiles, both halos)
and seg = 1 (no dif, a one-row tile); the parameters are seeded random numbers, not a trained state (the gcn weights of a
fresh SGN are zero, which would hide the g . x path)."""
import hashlib
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

# (V, seg, N, num_class, bias)
MODEL_CASES = [(15, 3, 1, 60, True), (15, 4, 1, 60, True), (15, 6, 1, 60, True), (25, 2, 1, 60, True), (2, 40, 1, 60, True),
               (3, 34, 1, 60, True), (7, 12, 2, 60, False), (32, 65, 3, 5, True), (15, 1, 1, 60, True)]
# (V, T, seg, S): four windows each, see sampler_windows
SAMPLER_CASES = [(15, 24, 20, 3), (25, 300, 20, 2), (2, 7, 5, 1)]
# the columns of a frames-tape row that the kernel writes (csrc/sgn_wgrad_plan.h: SgnFramesTape up to the end of dxn); the
# rest of a row is alignment padding that nothing writes or reads
FRAMES_TAPE_USED = 3 * 256 + 2 * 128 + 256 + 3 * 128 + 512 + 3 * 128 + 64 + 8 + 6


def sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()[:16]


def seeded_model(V, seg, num_class, bias, seed, dev):
    from agcn_amd.model.sgn import SGN
    model = SGN(num_class=num_class, num_point=V, seg=seg, bias=bias)
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in sorted(list(model.named_parameters()) + list(model.named_buffers())):
            if name in ('spa', 'tem') or not p.dtype.is_floating_point:
                continue
            r = torch.randn(p.shape, generator=gen)
            if name.endswith('running_var'):
                p.copy_(0.5 + r.abs())
            elif p.dim() > 1:
                p.copy_(r * math.sqrt(2.0 / p[0].numel()))
            elif '.bn' in name and name.endswith('weight'):
                p.copy_(1.0 + 0.25 * r)
            else:
                p.copy_(0.1 * r)
    return model.to(dev).eval()


def model_case(case, seed, dev, out):
    from agcn_amd import ops
    V, seg, N, nc, bias = case
    tag = f'v{V}_seg{seg}_n{N}' + ('' if bias else '_nobias')
    model = seeded_model(V, seg, nc, bias, seed, dev)
    gen = torch.Generator().manual_seed(seed + 1)
    x = torch.randn((N, seg, 3 * V), generator=gen).to(dev)
    cot = torch.randn((N, nc), generator=gen).to(dev)
    with torch.no_grad():
        wf, wc, wf_t, wc_t = model._images(transposed=True)
        feat, g = ops.sgn_frames(x, wf, V)
        logits = ops.sgn_clip(feat, wc, nc)
        dfeat = ops.sgn_clip_bwd(feat, wc, wc_t, cot)
        dx = ops.sgn_frames_bwd(x, wf, wf_t, dfeat, V)
        dfeat_t, ctape = ops.sgn_clip_bwd_tape(feat, wc, wc_t, cot)
        dx_t, ftape = ops.sgn_frames_bwd_tape(x, wf, wf_t, dfeat_t, V)
        rows = [('fwd feat', feat), ('fwd g', g), ('fwd logits', logits), ('bwd dfeat', dfeat), ('bwd dx', dx),
                ('tape dfeat', dfeat_t), ('tape dx', dx_t), ('tape clip', ctape),
                ('tape frames', ftape.view(N * seg * V, -1)[:, :FRAMES_TAPE_USED])]
        for rps in (0, 7):
            rows.append((f'wgrad d_wf rps{rps}', ops.sgn_frames_wgrad(x, wf, ftape, V, nc, rps)))
            rows.append((f'wgrad d_wc rps{rps}', ops.sgn_clip_wgrad(ctape, dfeat_t, cot, wc, V, rps)))
    torch.cuda.synchronize()
    for name, t in rows:
        out.append(f'{tag:24s} {name:20s} {sha(t)}')


def sampler_windows(V, T, gen):
    """Four windows (4, 3, T, V, 2): dense; null rows scattered and the second body absent from half of the frames; empty;
    three kept rows (fewer than any seg used here: the sampler pads)."""
    win = torch.randn((4, 3, T, V, 2), generator=gen)
    null = torch.rand((T, 2), generator=gen) < 0.3
    null[T // 2:, 1] = True
    win[1] = win[1] * (~null)[None, :, None, :]
    win[2] = 0
    keep = torch.zeros((T, 2), dtype=torch.bool)
    keep[0, 1] = keep[T // 2, 0] = keep[T - 1, 0] = True
    win[3] = win[3] * keep[None, :, None, :]
    return win


def sampler_case(case, seed, dev, out):
    from agcn_amd import ops
    V, T, seg, S = case
    tag = f'sample_v{V}_t{T}_seg{seg}_s{S}'
    gen = torch.Generator().manual_seed(seed)
    win = sampler_windows(V, T, gen).to(dev)
    r = torch.randint(-(1 << 31), 1 << 31, (4, S, seg), generator=gen, dtype=torch.int64).to(torch.int32).to(dev)  # all 32 bits
    dout = torch.randn((4, S, seg, 3 * V), generator=gen).to(dev)
    res, L = ops.sgn_sample(win, r, seg)
    dwin = ops.sgn_sample_bwd(win, r, dout, seg)
    torch.cuda.synchronize()
    for name, t in (('out', res), ('L', L), ('dwin', dwin)):
        out.append(f'{tag:24s} {name:20s} {sha(t)}')


def main():
    import agcn_amd  # noqa: F401
    dev = torch.device('cuda:0')
    lines = []
    for i, case in enumerate(MODEL_CASES):
        model_case(case, 4100 + 10 * i, dev, lines)
    for i, case in enumerate(SAMPLER_CASES):
        sampler_case(case, 4300 + i, dev, lines)
    print('\n'.join(lines))


if __name__ == '__main__':
    main()
