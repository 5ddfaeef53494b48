"""The eval-mode BatchNorm backward (agcn_bn_bwd_eval [+ _finalize]) against the two-pass train-mode one (agcn_bn_bwd_reduce
+ agcn_bn_bwd_apply_ex) on the same buffers, at the l2 shape (N'=128, C=64, P=7500) and the l9 shape (C=256, P=1875):
one and two branches, with and without the parameter sums.
    python tools/bench_bn_eval.py [--calls 30] [--rounds 3]
Every figure is the median over --calls device-event-timed calls after a warm-up; the variants alternate inside a round
and the whole measurement is repeated --rounds times in the process (the spread of the medians is the run-to-run
figure).  Bytes = the activation-sized passes each variant needs (fp32 tensors; the sign-bit mask adds 1/32 of one)."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import agcn_amd  # noqa: E402,F401
from agcn_amd import ops  # noqa: E402

SHAPES = {'l2': (128, 64, 300, 25), 'l9': (128, 256, 75, 25)}
# activation-sized passes (reads + writes): train = reduce + apply
PASSES = {('train', 1): 5, ('train', 2): 8, ('eval', 1): 3, ('eval', 2): 5, ('eval_nosums', 1): 2, ('eval_nosums', 2): 3}


def timed(fn, calls):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=30)
    ap.add_argument('--rounds', type=int, default=3)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    g = torch.Generator(dev).manual_seed(0)
    for sname, (N, C, T, V) in SHAPES.items():
        r = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
        y1, y2, dout = r(N, C, T, V), r(N, C, T, V), r(N, C, T, V)
        par = [(r(C) * 0.3 + 1, r(C) * 0.1, r(C) * 0.1, torch.rand(C, device=dev, generator=g) + 0.5) for _ in range(2)]
        ev = [ops.bn_eval_coeffs(*p) for p in par]
        tr = []
        for (gam, bet, _, _), y in zip(par, (y1, y2)):
            part = torch.stack([y.sum((0, 2, 3)), (y * y).sum((0, 2, 3))]).view(1, 2, C).contiguous()
            tr.append(ops.bn_train_coeffs(part, N * T * V, gam, bet, torch.zeros(C, device=dev), torch.ones(C, device=dev)))
        out, bits = ops.bn_act_fwd(y1, ev[0], y2, ev[1], relu=True, want_bits=True)
        del out
        amax = torch.empty(1, device=dev)
        tensor_bytes = N * C * T * V * 4
        for nb in (1, 2):
            two = nb == 2
            variants = {
                'train': lambda: ops.bn_bwd(dout, bits, y1, par[0][0], tr[0], y2 if two else None,
                                            par[1][0] if two else None, tr[1] if two else None, amax_out=amax),
                'eval': lambda: ops.bn_bwd_eval(dout, bits, y1, ev[0], y2 if two else None, ev[1] if two else None,
                                                want_sums=True, amax_out=amax),
                'eval_nosums': lambda: ops.bn_bwd_eval(dout, bits, None, ev[0], None, ev[1] if two else None,
                                                       want_sums=False, amax_out=amax),
            }
            for fn in variants.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            meds = {k: [] for k in variants}
            for _ in range(args.rounds):
                for k, fn in variants.items():
                    meds[k].append(statistics.median(timed(fn, args.calls)))
            base = statistics.median(meds['train'])
            for k, m in meds.items():
                med = statistics.median(m)
                bw = PASSES[(k, nb)] * tensor_bytes / (med * 1e-3) / 1e12
                print('%s C=%d P=%d branches=%d %-12s %.3f ms (rounds min %.3f max %.3f) %d passes %.2f TB/s  x%.2f vs train'
                      % (sname, C, T * V, nb, k, med, min(m), max(m), PASSES[(k, nb)], bw, base / med), flush=True)


if __name__ == '__main__':
    main()
