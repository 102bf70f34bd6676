#!/usr/bin/env python3
"""Time the loss layers of the training graph (mnc_amd/losses.py; csrc/loss.hip) in this process and run, per shape: the numpy
statement on this machine's CPU; torch-CPU's cross_entropy / smooth_l1_loss / binary_cross_entropy_with_logits with autograd, the
code a user writes today and so the yardstick; the host-array device call with its copies; the kernels alone between the HIP
event pairs of the context's launch profile; and one mnc_eltwise launch of the same element count in the same run, the floor
any launch pays.  Shapes: rpn_loss_cls [1, 2, 9*38, 63] with 256 valid labels, rpn_loss_bbox [1, 36, 38, 63] with sigma 3, and the
three head losses [R, 21], [R, 84], [R, 441] at R = 64 and R = 300.  Medians over --iters device rounds and --host-iters host rounds
after one warm-up each.  The gradients are compared; nothing about speed is asserted.
Prints one JSON line and writes it, under a heading, to --profile (default profiles/loss_bench.txt; "" writes nothing).

    python tools/loss_bench.py [--iters 20] [--host-iters 5] [--profile FILE]
"""
import os

import numpy as np

from _task_harness import emit, median_ms, parser

HEADING = """tools/loss_bench.py --iters %d --host-iters %d on one MI355X.  Per shape: numpy_ms = the float32 statement of mnc_amd/losses.py on
this machine's CPU; torch_ms = torch-CPU float32, loss and backward (the yardstick); device_ms = the host-array call, copies
included; kernels_us = the launches alone between the HIP event pairs of the context's profile (softmax: forward + finalize +
gradient; the others: one kernel + finalize); eltwise_us = one mnc_eltwise launch of the same element count in the same run, the
floor of any launch.  grad_equals_numpy: the device's gradient has the statement's bytes.  All sides in one process and run.

"""
LOSS_LAUNCHES = ("softmax_loss_fwd", "softmax_loss_grad", "smooth_l1_loss", "sigmoid_ce_loss", "loss_finalize")


def median(values):
    return round(sorted(values)[len(values) // 2], 2) if values else None


def launches_us(fn, rounds, names):
    from mnc_amd import backward as B
    out = []
    for _ in range(max(rounds, 1)):
        out.append(sum(ms for n, ms in B.kernel_times(fn) if n in names) * 1e3)
    return median(out)


def eltwise_us(count, rounds):
    """One mnc_eltwise (ReLU) launch over count elements on the same context: its microseconds, median."""
    from mnc_amd import backward as B
    with B.Session() as s:
        d_in, d_out = s.put(np.zeros(count, np.float32)), s.empty(count * 4)
        run = lambda: s.call("mnc_eltwise", d_in, d_out, count, 1)      # noqa: E731
        run()
        return launches_us(run, rounds, ("eltwise",))


def cases(rng):
    """-> [(name, numpy statement, torch function, device function, element count)], every function without arguments."""
    import torch
    import torch.nn.functional as F
    from mnc_amd import losses as L
    f = np.float32
    out = []

    def softmax(name, score, label):
        ts, tl = torch.tensor(score), torch.tensor(label.astype(np.int64)).reshape((score.shape[0],) + score.shape[2:])

        def torch_fn():
            x = ts.clone().requires_grad_(True)
            F.cross_entropy(x, tl, ignore_index=-1, reduction="mean").backward()
            return x.grad
        out.append((name, lambda: L.softmax_loss_numpy(score, label, -1), torch_fn, lambda: L.softmax_loss(score, label, -1), score.size))

    H, W = 38, 63
    label = np.full(9 * H * W, -1, f)
    label[rng.choice(label.size, 256, replace=False)] = rng.integers(0, 2, 256)
    softmax("rpn_loss_cls", f(rng.standard_normal((1, 2, 9 * H, W))), label.reshape(1, 1, 9 * H, W))

    def smooth(name, shape, sigma):
        pred, target = f(rng.standard_normal(shape)), f(rng.standard_normal(shape))
        w_in, w_out = f(rng.random(shape) < 0.25), f(rng.random(shape) < 0.25) / f(64)
        tp, tt, ti, to = (torch.tensor(a) for a in (pred, target, w_in, w_out))

        def torch_fn():
            x = tp.clone().requires_grad_(True)
            ((F.smooth_l1_loss(x * ti, tt * ti, beta=1.0 / sigma ** 2, reduction="none") * to).sum() / shape[0]).backward()
            return x.grad
        out.append((name, lambda: L.smooth_l1_loss_numpy(pred, target, w_in, w_out, sigma), torch_fn,
                    lambda: L.smooth_l1_loss(pred, target, w_in, w_out, sigma), pred.size))

    smooth("rpn_loss_bbox", (1, 36, H, W), 3.0)
    for R in (64, 300):
        softmax("loss_cls_%d" % R, f(rng.standard_normal((R, 21)) * 2), f(rng.integers(0, 21, R)))
        smooth("loss_bbox_%d" % R, (R, 84), 1.0)
        x, t = f(rng.standard_normal((R, 441)) * 2), f(rng.random((R, 1, 21, 21)) < 0.4)
        w = np.repeat(f(np.arange(R) < R // 4), 441).reshape(R, 1, 21, 21)
        tx, tt, tw = torch.tensor(x), torch.tensor(t.reshape(R, 441)), torch.tensor(w.reshape(R, 441))

        def torch_fn(tx=tx, tt=tt, tw=tw, R=R):
            v = tx.clone().requires_grad_(True)
            ((F.binary_cross_entropy_with_logits(v, tt, reduction="none") * tw).sum() / R).backward()
            return v.grad
        out.append(("loss_mask_%d" % R, lambda x=x, t=t, w=w: L.sigmoid_ce_loss_numpy(x, t, w), torch_fn,
                    lambda x=x, t=t, w=w: L.sigmoid_ce_loss(x, t, w), x.size))
    return out


def main():
    ap = parser()
    ap.set_defaults(iters=20, host_iters=5)
    ap.add_argument("--profile", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "loss_bench.txt"))
    args = ap.parse_args()
    import mnc_amd
    mnc_amd.install_paths()
    import torch
    torch.set_grad_enabled(True)
    line = {"workload": "SoftmaxWithLoss, SmoothL1Loss and SigmoidCrossEntropyLoss of mnc_5stage/train.prototxt: loss and gradient",
            "device_rounds": max(args.iters, 1), "host_rounds": max(args.host_iters, 1)}
    for name, numpy_fn, torch_fn, device_fn, count in cases(np.random.default_rng(25)):
        want, got = numpy_fn(), device_fn()
        torch_grad = torch_fn().numpy().reshape(want.grad.shape)
        line.update({name + "_grad_equals_numpy": bool(got.grad.tobytes() == want.grad.tobytes()),
                     name + "_grad_max_abs_diff_to_torch": float(np.abs(got.grad - torch_grad).max()),
                     name + "_loss": float(got.loss), name + "_loss_numpy": float(want.loss),
                     name + "_numpy_ms": median_ms(numpy_fn, args.host_iters)[0], name + "_torch_ms": median_ms(torch_fn, args.host_iters)[0],
                     name + "_device_ms": median_ms(device_fn, args.iters)[0],
                     name + "_kernels_us": launches_us(device_fn, args.iters, LOSS_LAUNCHES),
                     name + "_eltwise_us": eltwise_us(count, args.iters)})
    emit(line, HEADING % (max(args.iters, 1), max(args.host_iters, 1)), args.profile)


if __name__ == "__main__":
    main()
