#!/usr/bin/env python3
"""The KKT operator from stored value runs, top = (H + diag dx) v + J^T w, bottom = J v - diag(dc) w, of a batch: one launch
(hipnlp_kkt_times_device) against the composition a build without it offers, timed with HIP events (torch.cuda.Event), one event between
consecutive repetitions of a leg; varying-first handles, both diagonals present.

    A = hipnlp_kkt_times_device                                                      (ONE launch)
    B = hipnlp_hess_times_device + hipnlp_jac_times_device + hipnlp_jac_transpose_times_device (no gradient)
        + torch.add, torch.addcmul, torch.addcmul into preallocated tensors          (SIX launches)
    C = A against the 8-byte words it must move at 8 TB/s: both value runs once, v, w, dx, dc in, top and bottom out
    D = hipnlp_hess_times_device alone
    E = hipnlp_jac_times_device alone (J v only)
    F = hipnlp_jac_transpose_times_device alone (no gradient)

Every leg is timed in `--rounds` rounds of `--launches` repetitions after a warm-up, the legs alternating within a round in one process; a
round's figure is the median of its repetitions (microseconds).  The claim to check: every round of A below every round of B at every
shape, one box, one session.  The outputs of A and B are compared once per shape (torch.addcmul rounds the product before the addition,
A uses one fused multiply-add: close, not the same bits; the bitwise statements are those of tests/test_gpu_kkt_operator.py)."""
import argparse
import os
import socket
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = ("planar_100x1", "planar_100x64", "planar_100x1024", "stairs_200x16")


def make_shape(name, model):
    from hippopt_amd.kinodyn_settings import periodic_step_settings, stairs_settings
    from hippopt_amd.synthetic import make_workload, place_on_step_flanks
    if name.startswith("planar"):
        N, B = 100, int(name.split("x")[1])
        st = periodic_step_settings(N, model)
    else:
        N, B = 200, 16
        st = stairs_settings(N, model)
    x, p = make_workload(st, model, batch=B, seed=1234)
    if not name.startswith("planar"):
        place_on_step_flanks(x[:2], st, seed=5)
    return st, x, p


def event_times(torch, fn, count):
    """per-repetition microseconds of `count` consecutive calls of fn, an event between every two"""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(count + 1)]
    ev[0].record()
    for i in range(count):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    return np.array([ev[i].elapsed_time(ev[i + 1]) * 1000.0 for i in range(count)])


def probe(shape, rounds, launches, warmup):
    # (every launch and every event on one explicit stream: a NULL stream would be the handle's own to the library)
    import torch
    work = torch.cuda.Stream()
    with torch.cuda.stream(work):
        return probe_on(shape, rounds, launches, warmup, work.cuda_stream)


def probe_on(shape, rounds, launches, warmup, stream):
    import torch
    from hippopt_amd import hipnlp
    from hippopt_amd.robot_model import synthetic_ergocub
    model = synthetic_ergocub()
    st, x, p = make_shape(shape, model)
    B = x.shape[0]
    eng = hipnlp.HipNlp(st, model, batch=B, jac_varying_first=True)
    eng.set_params(p)
    n, m, nnz, nnz_h = eng.n, eng.m, eng.nnz, eng.hess_nnz()
    dev = "cuda"
    rng = np.random.RandomState(7)
    t = lambda a: torch.tensor(a, dtype=torch.float64, device=dev)  # noqa: E731
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev)  # noqa: E731
    xd, sig, lam = t(x), t(rng.uniform(0.5, 1.5, B)), t(rng.standard_normal((B, m)))
    v, w = t(rng.standard_normal((B, n))), t(rng.standard_normal((B, m)))
    dx, dc = t(rng.uniform(0.1, 3.0, (B, n))), t(rng.uniform(0.1, 3.0, (B, m)))
    jac, hess = z(B, nnz), z(B, nnz_h)
    top, bottom, hv, jt, s, jv, top_b, bottom_b = z(B, n), z(B, m), z(B, n), z(B, n), z(B, n), z(B, m), z(B, n), z(B, m)
    eng.eval_device(xd.data_ptr(), 0, 0, 0, jac.data_ptr(), stream=stream)
    eng.eval_hess_device(xd.data_ptr(), sig.data_ptr(), lam.data_ptr(), hess.data_ptr(), stream=stream)
    torch.cuda.synchronize()

    def leg_a():
        eng.kkt_times_device(hess.data_ptr(), jac.data_ptr(), v.data_ptr(), w.data_ptr(), top.data_ptr(), bottom.data_ptr(), dx_ptr=dx.data_ptr(), dc_ptr=dc.data_ptr(), stream=stream)

    def hess_times():
        eng.hess_times_device(hess.data_ptr(), v.data_ptr(), hv.data_ptr(), stream=stream)

    def jac_times():
        eng.jac_times_device(jac.data_ptr(), v.data_ptr(), jv.data_ptr(), stream=stream)

    def transpose():
        eng.jac_transpose_times_device(jac.data_ptr(), w.data_ptr(), jt.data_ptr(), stream=stream)

    def leg_b():
        hess_times()
        jac_times()
        transpose()
        torch.add(hv, jt, out=s)
        torch.addcmul(s, dx, v, out=top_b)
        torch.addcmul(jv, dc, w, value=-1.0, out=bottom_b)

    parts = {"A": leg_a, "B": leg_b, "D": hess_times, "E": jac_times, "F": transpose}
    for name in parts:
        for _ in range(warmup):
            parts[name]()
    torch.cuda.synchronize()
    res = {k: [] for k in parts}
    for _ in range(rounds):
        for name in parts:
            res[name].append(float(np.median(event_times(torch, parts[name], launches))))
    leg_a()
    leg_b()
    torch.cuda.synchronize()
    return {"shape": shape, "batch": B, "N": st.horizon_length, "n": n, "m": m, "nnz": nnz, "nnz_h": nnz_h, "rounds": res,
            "max_abs_diff_top": float((top - top_b).abs().max()), "max_abs_diff_bottom": float((bottom - bottom_b).abs().max()),
            "top_bits_equal": bool(torch.equal(top.view(torch.int64), top_b.view(torch.int64))),
            "bottom_bits_equal": bool(torch.equal(bottom.view(torch.int64), bottom_b.view(torch.int64)))}


def report(recs, session):
    lines = ["KKT operator from stored value runs: one launch of hipnlp_kkt_times_device (A) against the three launches it replaces + three torch element-wise kernels (B)",
             "tools/kkt_operator_probe.py; box %s, session %s; one box, one session; microseconds per repetition, median of each round" % (socket.gethostname(), session), ""]
    ok = True
    fmt = lambda ts: " ".join("%.1f" % t for t in ts)  # noqa: E731
    for r in recs:
        rr = r["rounds"]
        gate = max(rr["A"]) < min(rr["B"])
        ok &= gate
        words = r["nnz_h"] + r["nnz"] + 3 * r["n"] + 3 * r["m"]          # both value runs, v, dx, top, w, dc, bottom
        floor = 8.0 * words * r["batch"] / 8e12 * 1e6
        med = {k: float(np.median(rr[k])) for k in rr}
        lines.append("%s (N = %d, B = %d, n = %d, m = %d, nnz = %d, nnz_h = %d; varying-first handle)" % (r["shape"], r["N"], r["batch"], r["n"], r["m"], r["nnz"], r["nnz_h"]))
        lines.append("  A  (kkt_times_device, one launch)                 median %8.1f   rounds: %s" % (med["A"], fmt(rr["A"])))
        lines.append("  B  (three launches + add, addcmul, addcmul)       median %8.1f   rounds: %s" % (med["B"], fmt(rr["B"])))
        lines.append("  D  (hess_times_device alone)                      median %8.1f   rounds: %s" % (med["D"], fmt(rr["D"])))
        lines.append("  E  (jac_times_device alone, J v)                  median %8.1f   rounds: %s" % (med["E"], fmt(rr["E"])))
        lines.append("  F  (jac_transpose_times_device alone, J^T w)      median %8.1f   rounds: %s" % (med["F"], fmt(rr["F"])))
        lines.append("  A / B = %.3f;  A / (D + E + F) = %.3f (medians of the rounds)" % (med["A"] / med["B"], med["A"] / (med["D"] + med["E"] + med["F"])))
        lines.append("  C: A = %.1f against %.2f for 8 (nnz_h + nnz + 3 n + 3 m) = %d bytes per trajectory at 8 TB/s: %.1f x" % (med["A"], floor, 8 * words, med["A"] / floor))
        lines.append("  every A round below every B round: %s" % ("yes" if gate else "NO"))
        lines.append("  outputs of A and B: max |top| diff %.3e (bits equal: %s), max |bottom| diff %.3e (bits equal: %s)"
                     % (r["max_abs_diff_top"], r["top_bits_equal"], r["max_abs_diff_bottom"], r["bottom_bits_equal"]))
        lines.append("")
    lines.append("EVERY A ROUND BELOW EVERY B ROUND AT EVERY SHAPE" if ok else "A IS NOT BELOW B AT EVERY SHAPE")
    return "\n".join(lines) + "\n", ok


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out")
    ap.add_argument("--session", default=time.strftime("%Y-%m-%d %H:%M:%S"))
    a = ap.parse_args()
    recs = []
    for shape in a.shapes.split(","):
        recs.append(probe(shape, a.rounds, a.launches, a.warmup))
        print(recs[-1]["shape"], {k: ["%.1f" % t for t in v] for k, v in recs[-1]["rounds"].items()}, flush=True)
    text, _ = report(recs, a.session)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
