"""``pre_normalization`` of skeleton data on the GPU (reference ``data_gen/preprocess.py``): pad the null frames of
every body with its valid ones, centre every frame on the first body's joint 1, rotate the clip so that the bone
``zaxis`` of the first body's first frame lies on z and the bone ``xaxis`` on x.  One HIP kernel, one workgroup per
sample (``ops.prenorm`` / csrc/prenorm.hip); the reference loops over samples, bodies, frames and joints in Python.

Deviation, by design: a frame (joint) is null iff ALL its values are zero.  The reference tests ``sum() == 0``, which
also fires on a non-null frame or joint whose values cancel to exactly zero."""
from . import ops


def pre_normalization(data, zaxis=[0, 1], zaxis2=None, xaxis=[8, 4], pad=True, center=True, center_firstframe=False):
    """data (N, C=3, T, V, M) fp32 on the GPU -> the normalised tensor of the same shape (a new tensor; the input is
    left as it is).  Signature and defaults of the reference, minus ``verbose`` and ``tqdm``."""
    if data.dim() != 5 or data.shape[1] != 3:
        raise ValueError(f"agcn_amd: pre_normalization takes (N, 3, T, V, M), got {tuple(data.shape)}")
    raw = data.permute(0, 4, 2, 3, 1).contiguous()          # N, M, T, V, C: the order the reference works in
    out, _, _ = ops.prenorm(raw, zaxis=zaxis, zaxis2=zaxis2, xaxis=xaxis, pad=pad, center=center,
                            center_firstframe=center_firstframe)
    return out
