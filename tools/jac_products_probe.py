#!/usr/bin/env python3
"""Products with a stored value run of jac g (hipnlp_jac_times_device, hipnlp_jac_transpose_times_device) of a batch, timed with HIP
events (torch.cuda.Event), one event between consecutive repetitions of a leg; varying-first handles.

    A = hipnlp_eval_device (grad f + jac g into HBM) + hipnlp_jac_times_device (J v and grad f . v)
    B = the same evaluation + the better of   a torch.sparse CSR mat-vec, block diagonal over the batch (values gathered into row order)
                                               an index_add_ over the triplets
        each with (grad f * v).sum(1) — entry points a build without the two products has
    C = hipnlp_jac_times_device alone             (reported against the bytes it must move, not gated)
    D = hipnlp_jac_transpose_times_device alone   (likewise)
    E = hipnlp_eval_lagrangian_grad_device        (the fused launch that re-runs the knot program: what D replaces at a fixed x)

Every leg is timed in `--rounds` rounds of `--launches` repetitions after a warm-up, the legs alternating within a round; a round's figure
is the median of its repetitions (microseconds).  The acceptance for speed: every round of A below every round of B, one box, one
session.  C and D are read against 8 bytes per word they must move at 8 TB/s: the value run once, the vectors in and out."""
import argparse
import os
import socket
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = ("planar_100x64", "planar_100x1024", "stairs_200x16")


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
    n, m, nnz = eng.n, eng.m, eng.nnz
    dev = "cuda"
    xd = torch.tensor(x, device=dev)
    rng = np.random.RandomState(7)
    sig = torch.tensor(rng.uniform(0.5, 1.5, B), device=dev)
    lam = torch.tensor(rng.standard_normal((B, m)), device=dev)
    v = torch.tensor(rng.standard_normal((B, n)), device=dev)
    grad = torch.zeros((B, n), dtype=torch.float64, device=dev)
    jac = torch.zeros((B, nnz), dtype=torch.float64, device=dev)
    jv = torch.zeros((B, m), dtype=torch.float64, device=dev)
    dot = torch.zeros(B, dtype=torch.float64, device=dev)
    out = torch.zeros((B, n), dtype=torch.float64, device=dev)
    ir, jc = eng.sparsity()
    ir, jc = ir.astype(np.int64), jc.astype(np.int64)
    order = np.lexsort((jc, ir))                     # row order of the triplets: the CSR of J
    itype = torch.int32 if B * nnz < 2 ** 31 else torch.int64
    crow = torch.zeros(B * m + 1, dtype=torch.int64, device=dev)
    crow[1:] = torch.cumsum(torch.tensor(np.bincount(ir, minlength=m), device=dev).repeat(B), 0)
    col = (torch.arange(B, device=dev, dtype=torch.int64)[:, None] * n + torch.tensor(jc[order], device=dev)[None, :]).reshape(-1)
    crow, col = crow.to(itype), col.to(itype)
    order_t, ir_t, jc_t = torch.tensor(order, device=dev), torch.tensor(ir, device=dev), torch.tensor(jc, device=dev)
    vcol = v.reshape(-1, 1)

    def evaluate():
        eng.eval_device(xd.data_ptr(), 0, grad.data_ptr(), 0, jac.data_ptr(), stream=stream)

    def times():
        eng.jac_times_device(jac.data_ptr(), v.data_ptr(), jv.data_ptr(), dot.data_ptr(), grad_values_ptr=grad.data_ptr(), stream=stream)

    def leg_a():
        evaluate()
        times()

    def leg_b_csr():
        evaluate()
        a = torch.sparse_csr_tensor(crow, col, jac[:, order_t].reshape(-1), (B * m, B * n))
        jv.copy_(torch.sparse.mm(a, vcol).reshape(B, m))
        dot.copy_((grad * v).sum(1))

    def leg_b_index_add():
        evaluate()
        y = torch.zeros((B, m), dtype=torch.float64, device=dev)
        y.index_add_(1, ir_t, jac * v[:, jc_t])
        jv.copy_(y)
        dot.copy_((grad * v).sum(1))

    def transpose():
        eng.jac_transpose_times_device(jac.data_ptr(), lam.data_ptr(), out.data_ptr(), grad_values_ptr=grad.data_ptr(), obj_factor_ptr=sig.data_ptr(), stream=stream)

    def fused_lgrad():
        eng.eval_lagrangian_grad_device(xd.data_ptr(), sig.data_ptr(), lam.data_ptr(), out.data_ptr(), stream=stream)

    parts = {"A": leg_a, "B_csr": leg_b_csr, "B_index_add": leg_b_index_add, "C": times, "D": transpose, "E": fused_lgrad}
    evaluate()
    for name in list(parts):   # warm-up; a product that this torch build cannot run is left out and said so
        try:
            for _ in range(warmup):
                parts[name]()
            torch.cuda.synchronize()
        except RuntimeError as err:
            if not name.startswith("B_"):
                raise
            print("%s: %s: %s" % (shape, name, err), file=sys.stderr)
            del parts[name]
    res = {k: [] for k in parts}
    for _ in range(rounds):
        for name in parts:
            evaluate()
            res[name].append(float(np.median(event_times(torch, parts[name], launches))))
    rec = {"shape": shape, "batch": B, "N": st.horizon_length, "n": n, "m": m, "nnz": nnz, "rounds": res}
    rec["B"] = [min(t) for t in zip(*[res[k] for k in res if k.startswith("B_")])]
    # the vectors themselves agree
    leg_b_index_add()
    ref_jv, ref_dot = jv.clone(), dot.clone()
    leg_a()
    torch.cuda.synchronize()
    rec["max_abs_diff_jv"] = float((jv - ref_jv).abs().max())
    rec["max_abs_diff_dot"] = float((dot - ref_dot).abs().max())
    transpose()
    ref = out.clone()
    fused_lgrad()
    torch.cuda.synchronize()
    rec["max_abs_diff_D_vs_E"] = float((out - ref).abs().max())
    return rec


def report(recs, session):
    lines = ["Stored-values Jacobian products: evaluate + multiply with hipnlp_jac_times_device (A) against evaluate + torch (B); the two launches alone (C, D)",
             "tools/jac_products_probe.py; box %s, session %s; one box, one session; microseconds per repetition, median of each round" % (socket.gethostname(), session), ""]
    ok = True
    fmt = lambda ts: " ".join("%.1f" % t for t in ts)  # noqa: E731
    for r in recs:
        rr = r["rounds"]
        gate = max(rr["A"]) < min(r["B"])
        ok &= gate
        words_c = r["nnz"] + 2 * r["n"] + r["m"]          # the value run, v, grad f, J v
        words_d = r["nnz"] + 2 * r["n"] + r["m"]          # the value run, grad f, lambda, out
        floor_c, floor_d = (8.0 * w * r["batch"] / 8e12 * 1e6 for w in (words_c, words_d))
        lines.append("%s (N = %d, B = %d, n = %d, m = %d, nnz = %d; varying-first handle)" % (r["shape"], r["N"], r["batch"], r["n"], r["m"], r["nnz"]))
        lines.append("  A  (eval_device + jac_times_device)     rounds: %s" % fmt(rr["A"]))
        lines.append("  B  (eval_device + the better product)   rounds: %s" % fmt(r["B"]))
        for k in sorted(rr):
            if k.startswith("B_"):
                lines.append("    %-38s rounds: %s" % (k, fmt(rr[k])))
        lines.append("  C  (jac_times_device alone)             rounds: %s" % fmt(rr["C"]))
        lines.append("  D  (jac_transpose_times_device alone)   rounds: %s" % fmt(rr["D"]))
        lines.append("  E  (eval_lagrangian_grad_device)        rounds: %s" % fmt(rr["E"]))
        lines.append("  A / B = %.3f;  D / E = %.3f (medians of the rounds)" % (np.median(rr["A"]) / np.median(r["B"]), np.median(rr["D"]) / np.median(rr["E"])))
        lines.append("  C = %.1f against %.1f for 8 (nnz + 2 n + m) bytes per trajectory at 8 TB/s: %.1f x" % (np.median(rr["C"]), floor_c, np.median(rr["C"]) / floor_c))
        lines.append("  D = %.1f against %.1f for 8 (nnz + 2 n + m) bytes per trajectory at 8 TB/s: %.1f x" % (np.median(rr["D"]), floor_d, np.median(rr["D"]) / floor_d))
        lines.append("  every A round below every B round: %s" % ("yes" if gate else "NO"))
        lines.append("  max |J v (A) - J v (B)| = %.3e, max |dot (A) - dot (B)| = %.3e, max |D - E| = %.3e" % (r["max_abs_diff_jv"], r["max_abs_diff_dot"], r["max_abs_diff_D_vs_E"]))
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
