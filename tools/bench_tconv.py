"""Temporal convolution with any kernel size / stride / padding (agcn_tconv_*): one JSON line per case with the
forward, backward (data + weight) and total times, GB/s on the compulsory HBM bytes and TF/s.

    python tools/bench_tconv.py [--iters 20] [--warmup 5]

Cases: the windowed aagcn_vNN backbone layers at NTU batch 64 (N*M = 128, V = 25, k3/s3/p0: 3->16 and 16->16 with its
1x1 stride-3 residual on T = 300 input) and k = 3/5/7 stride 1 against k = 9 at the l2-4 (64 ch, T = 300) and l9
(256 ch, T = 75) shapes.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [
    # name, N, Cin, Cout, T, V, taps, stride, pad
    ('win_3_16_k3s3p0', 128, 3, 16, 300, 25, 3, 3, 0),
    ('win_16_16_k3s3p0', 128, 16, 16, 300, 25, 3, 3, 0),
    ('win_16_16_res_k1s3', 128, 16, 16, 300, 25, 1, 3, 0),
    ('l2_64_k3s1', 128, 64, 64, 300, 25, 3, 1, 1),
    ('l2_64_k5s1', 128, 64, 64, 300, 25, 5, 1, 2),
    ('l2_64_k7s1', 128, 64, 64, 300, 25, 7, 1, 3),
    ('l2_64_k9s1', 128, 64, 64, 300, 25, 9, 1, 4),
    ('l9_256_k3s1', 128, 256, 256, 75, 25, 3, 1, 1),
    ('l9_256_k5s1', 128, 256, 256, 75, 25, 5, 1, 2),
    ('l9_256_k7s1', 128, 256, 256, 75, 25, 7, 1, 3),
    ('l9_256_k9s1', 128, 256, 256, 75, 25, 9, 1, 4),
]


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    import agcn_amd  # noqa: F401
    from agcn_amd import lib, ops
    dev = torch.device('cuda:0')
    L = lib.load()
    for name, N, Cin, Cout, T, V, taps, stride, pad in CASES:
        g = torch.Generator(device=dev).manual_seed(1)
        x = torch.randn(N, Cin, T, V, device=dev, generator=g)
        w = torch.randn(Cout, Cin, taps, 1, device=dev, generator=g) * 0.1
        b = torch.zeros(Cout, device=dev)
        To = ops.conv_out_frames(T, taps, stride, pad)
        dy = torch.randn(N, Cout, To, V, device=dev, generator=g)
        x_amax, dy_amax = x.abs().max().reshape(1), dy.abs().max().reshape(1)
        fwd = lambda: ops.conv_fwd(x, w, b, stride, want_stats=True, x_amax=x_amax, pad=pad)  # noqa: E731
        bwd = lambda: (ops.conv_bwd_data(dy, w, tuple(x.shape), stride, dy_amax=dy_amax, pad=pad),  # noqa: E731
                       ops.conv_bwd_weight(dy, x, tuple(w.shape), stride, dy_amax, x_amax, pad=pad))
        fwd()
        kf = L.agcn_last_kernel().decode()
        bwd()
        kb = L.agcn_last_kernel().decode()
        t_f = timed(fwd, args.iters, args.warmup)
        t_b = timed(bwd, args.iters, args.warmup)
        xb, yb, wb = x.numel() * 4, dy.numel() * 4, w.numel() * 4
        bytes_f = xb + yb + wb                    # read x, w; write y
        bytes_b = (yb + wb + xb) + (yb + xb + wb)  # dx: read dy, w, write dx; dw: read dy, x, write dw
        flops = 2.0 * N * Cout * To * V * Cin * taps
        print(json.dumps({
            'case': name, 'N': N, 'Cin': Cin, 'Cout': Cout, 'T': T, 'V': V, 'taps': taps, 'stride': stride, 'pad': pad,
            'mode': L.agcn_gemm_mode().decode(), 'fwd_kernel': kf, 'bwd_data_kernel': kb,
            'fwd_ms': round(t_f, 4), 'bwd_ms': round(t_b, 4), 'total_ms': round(t_f + t_b, 4),
            'fwd_GBps': round(bytes_f / t_f / 1e6, 1), 'bwd_GBps': round(bytes_b / t_b / 1e6, 1),
            'fwd_TFps': round(flops / t_f / 1e9, 2), 'total_TFps': round(3 * flops / (t_f + t_b) / 1e9, 2)}),
            flush=True)


if __name__ == '__main__':
    main()
