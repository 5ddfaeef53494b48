"""Normalise a skeleton dataset on the GPU: the reference's ``data_gen`` step (``pre_normalization`` of the whole
``.npy`` array (N, 3, T, V, M) before training), in batches through ``agcn_amd.preprocess.pre_normalization``.
    python tools/prenorm_dataset.py IN.npy OUT.npy [--batch 256] [--zaxis 0 1] [--xaxis 8 4] [--zaxis2 A B]
                                    [--no-zaxis] [--no-xaxis] [--no-pad] [--center-firstframe]
The input is memory-mapped and the output written batch by batch, so neither has to fit in host memory."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('src')
    ap.add_argument('dst')
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--zaxis', type=int, nargs=2, default=[0, 1])
    ap.add_argument('--xaxis', type=int, nargs=2, default=[8, 4])
    ap.add_argument('--zaxis2', type=int, nargs=2, default=None)
    ap.add_argument('--no-zaxis', action='store_true')
    ap.add_argument('--no-xaxis', action='store_true')
    ap.add_argument('--no-pad', action='store_true')
    ap.add_argument('--center-firstframe', action='store_true')
    args = ap.parse_args()
    import agcn_amd  # noqa: F401
    from agcn_amd.preprocess import pre_normalization
    if not torch.cuda.is_available():
        raise SystemExit('prenorm_dataset needs a GPU: the normalisation has no CPU path')
    dev = torch.device('cuda:0')
    src = np.load(args.src, mmap_mode='r')
    if src.ndim != 5 or src.shape[1] != 3:
        raise SystemExit(f'expected an array (N, 3, T, V, M), got {src.shape}')
    dst = np.lib.format.open_memmap(args.dst, mode='w+', dtype=np.float32, shape=src.shape)
    t0 = time.perf_counter()
    for i in range(0, src.shape[0], args.batch):
        x = torch.from_numpy(np.ascontiguousarray(src[i:i + args.batch], dtype=np.float32)).to(dev)
        y = pre_normalization(x, zaxis=None if args.no_zaxis else args.zaxis, zaxis2=args.zaxis2,
                              xaxis=None if args.no_xaxis else args.xaxis, pad=not args.no_pad,
                              center=not args.center_firstframe, center_firstframe=args.center_firstframe)
        dst[i:i + args.batch] = y.cpu().numpy()
    dst.flush()
    dt = time.perf_counter() - t0
    print(f'{src.shape[0]} samples {tuple(src.shape[1:])} -> {args.dst} in {dt:.2f} s ({src.shape[0] / dt:.0f} samples/s, '
          f'file reads and writes included)')


if __name__ == '__main__':
    main()
