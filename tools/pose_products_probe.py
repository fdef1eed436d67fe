#!/usr/bin/env python3
"""The pose finder's products of a batch — xbar = sigma grad f + J^T lambda, (grad f . v, J v), H v — each in its one launch (A) against
"evaluate, store, multiply" through the API of a build WITHOUT them (B), timed with HIP events (torch.cuda.Event), one event between
consecutive launches.

    B (first order)  = hipnlp_pose_eval_device with grad f and jac g into HBM
                     + min(a torch.sparse CSR product, block diagonal over the batch; an index_add_ over the triplets)
    B (second order) = hipnlp_pose_eval_hess_device into HBM + the same two ways for the symmetric product
    C                = the launch each A derives from, alone: hipnlp_pose_eval_device (f, grad f, g, jac g) / hipnlp_pose_eval_hess_device

Every quantity is timed in `--rounds` rounds of `--launches` launches after a warm-up; a round's figure is the median of its launches
(microseconds).  B uses only entry points that a build of the parent commit has, so the same script times it on that build (--lib, --what B).

    python tools/pose_products_probe.py --lib NEW.so    --what A,B,C --json new.json
    python tools/pose_products_probe.py --lib PARENT.so --what B     --json parent.json
    python tools/pose_products_probe.py --summarize new.json parent.json --out report.txt"""
import argparse
import json
import os
import socket
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for q in (ROOT, os.path.join(ROOT, "tests")):
    if q not in sys.path:
        sys.path.insert(0, q)

SHAPES = ("planar_4096", "planar_16384", "steps_4096")
PRODUCTS = ("lgrad", "jvp", "hvp")


def event_times(torch, fn, count):
    """per-launch microseconds of `count` consecutive calls of fn, an event between every two"""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(count + 1)]
    ev[0].record()
    for i in range(count):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    return np.array([ev[i].elapsed_time(ev[i + 1]) * 1000.0 for i in range(count)])


def probe(lib_path, shape, what, rounds, launches, warmup):
    import torch
    work = torch.cuda.Stream()   # (every launch and every event on one explicit stream: a NULL stream would be the handle's own)
    with torch.cuda.stream(work):
        return probe_on(lib_path, shape, what, rounds, launches, warmup, work.cuda_stream)


def block_csr(torch, rows, cols, n_rows, n_cols, B, dev):
    """CSR structure of the block-diagonal matrix of B copies of a pattern, and the order that brings a value run into it"""
    order = np.lexsort((cols, rows))
    counts = torch.tensor(np.bincount(rows, minlength=n_rows), device=dev)
    crow = torch.zeros(B * n_rows + 1, dtype=torch.int64, device=dev)
    crow[1:] = torch.cumsum(counts.repeat(B), 0)
    col = (torch.arange(B, device=dev, dtype=torch.int64)[:, None] * n_cols + torch.tensor(cols[order], device=dev)[None, :]).reshape(-1)
    ident = bool(np.array_equal(order, np.arange(order.size)))
    return crow, col, None if ident else torch.tensor(order, device=dev), (B * n_rows, B * n_cols)


def probe_on(lib_path, shape, what, rounds, launches, warmup, stream):
    import torch
    from hippopt_amd import hipnlp
    from hippopt_amd.pose_settings import make_pose_workload
    from hippopt_amd.robot_model import synthetic_ergocub
    from test_pose_body_hostemu import variants
    hipnlp._LIB_PATH = lib_path                     # (this process binds the library under test and no other)
    model = synthetic_ergocub()
    kind, B = shape.split("_")
    B = int(B)
    st = variants(model)["default" if kind == "planar" else "steps"]
    x3, p3 = make_pose_workload(st, model, 64, 1234)
    cyc = np.arange(B) % 64
    eng = hipnlp.HipPose(st, model, batch=B)
    eng.set_params(p3[cyc])
    n, m, nnz = eng.n, eng.m, eng.nnz
    hr, hc = (a.astype(np.int64) for a in eng.hess_sparsity())
    ir, jc = (a.astype(np.int64) for a in eng.sparsity())
    hnnz = hr.size
    dev = "cuda"
    rng = np.random.RandomState(7)
    xd = torch.tensor(x3[cyc], device=dev)
    sig = torch.tensor(rng.uniform(0.5, 1.5, B), device=dev)
    lam = torch.tensor(rng.standard_normal((B, m)), device=dev)
    v = torch.tensor(rng.standard_normal((B, n)), device=dev)
    f, grad, g, jac = (torch.zeros(s, dtype=torch.float64, device=dev) for s in ((B,), (B, n), (B, m), (B, nnz)))
    vals = torch.zeros((B, hnnz), dtype=torch.float64, device=dev)
    out, jv, dot = (torch.zeros(s, dtype=torch.float64, device=dev) for s in ((B, n), (B, m), (B,)))
    ir_t, jc_t, hr_t, hc_t = (torch.tensor(a, device=dev) for a in (ir, jc, hr, hc))
    off = np.flatnonzero(hr != hc)
    off_t = torch.tensor(off, device=dev)
    jt = block_csr(torch, jc, ir, n, m, B, dev)        # J^T: rows are columns of jac g
    jn = block_csr(torch, ir, jc, m, n, B, dev)        # J
    hu = block_csr(torch, hc, hr, n, n, B, dev)        # upper triangle with the diagonal: the transposed triplets
    hl = block_csr(torch, hr[off], hc[off], n, n, B, dev)

    def spmm(struct, values, vec):
        crow, col, order, size = struct
        a = torch.sparse_csr_tensor(crow, col, (values if order is None else values[:, order]).reshape(-1), size)
        return torch.sparse.mm(a, vec.reshape(-1, 1))

    def eval_all():
        eng.eval_device(xd.data_ptr(), f.data_ptr(), grad.data_ptr(), g.data_ptr(), jac.data_ptr(), stream=stream)

    def eval_hess():
        eng.eval_hess_device(xd.data_ptr(), sig.data_ptr(), lam.data_ptr(), vals.data_ptr(), stream=stream)

    legs = {
        "B_eval": eval_all, "B_eval_hess": eval_hess,
        "B_lgrad_csr": lambda: out.copy_((sig[:, None] * grad) + spmm(jt, jac, lam).reshape(B, n)),
        "B_lgrad_index_add": lambda: out.copy_((sig[:, None] * grad).index_add_(1, jc_t, jac * lam[:, ir_t])),
        "B_jvp_csr": lambda: (jv.copy_(spmm(jn, jac, v).reshape(B, m)), dot.copy_((grad * v).sum(1))),
        "B_jvp_index_add": lambda: (jv.copy_(torch.zeros_like(jv).index_add_(1, ir_t, jac * v[:, jc_t])), dot.copy_((grad * v).sum(1))),
        "B_hvp_csr": lambda: out.copy_((spmm(hu, vals, v) + spmm(hl, vals[:, off_t], v)).reshape(B, n)),
        "B_hvp_index_add": lambda: out.copy_(torch.zeros_like(out).index_add_(1, hr_t, vals * v[:, hc_t]).index_add_(1, hc_t[off_t], vals[:, off_t] * v[:, hr_t[off_t]])),
        "A_lgrad": lambda: eng.eval_lagrangian_grad_device(xd.data_ptr(), sig.data_ptr(), lam.data_ptr(), out.data_ptr(), stream=stream),
        "A_jvp": lambda: eng.eval_jac_vec_device(xd.data_ptr(), v.data_ptr(), dot.data_ptr(), jv.data_ptr(), stream=stream),
        "A_hvp": lambda: eng.eval_hess_vec_device(xd.data_ptr(), sig.data_ptr(), lam.data_ptr(), v.data_ptr(), out.data_ptr(), stream=stream),
        "C_eval": eval_all, "C_eval_hess": eval_hess,
    }
    parts = {k: fn for k, fn in legs.items() if k[0] in what}
    eval_all()
    eval_hess()
    for name in list(parts):   # warm-up; a product that this torch build cannot run is left out and said so
        try:
            for _ in range(warmup):
                parts[name]()
            torch.cuda.synchronize()
        except RuntimeError as err:
            if not name.startswith("B_") or name in ("B_eval", "B_eval_hess"):
                raise
            print("%s: %s: %s" % (shape, name, err), file=sys.stderr)
            del parts[name]
    res = {k: [] for k in parts}
    for _ in range(rounds):
        for name in parts:
            res[name].append(float(np.median(event_times(torch, parts[name], launches))))
    rec = {"shape": shape, "batch": B, "n": n, "m": m, "nnz": nnz, "hnnz": int(hnnz), "lib": lib_path, "rounds": res}
    if "B" in what:
        for prod in PRODUCTS:
            ways = [res[k] for k in res if k.startswith("B_%s_" % prod)]
            base = res["B_eval_hess" if prod == "hvp" else "B_eval"]
            rec["B_" + prod] = [b + min(w) for b, w in zip(base, zip(*ways))]
    if "A" in what and "B" in what:   # the vectors themselves agree
        eval_all()
        eval_hess()
        legs["B_lgrad_index_add"]()
        ref = out.clone()
        legs["A_lgrad"]()
        torch.cuda.synchronize()
        rec["max_abs_diff_lgrad"] = float((out - ref).abs().max())
        legs["B_hvp_index_add"]()
        ref = out.clone()
        legs["A_hvp"]()
        torch.cuda.synchronize()
        rec["max_abs_diff_hvp"] = float((out - ref).abs().max())
        legs["B_jvp_index_add"]()
        ref, refd = jv.clone(), dot.clone()
        legs["A_jvp"]()
        torch.cuda.synchronize()
        rec["max_abs_diff_jvp"] = float(max((jv - ref).abs().max(), (dot - refd).abs().max()))
    return rec


def summarize(new_path, parent_path, out_path, session):
    new, par = json.load(open(new_path)), json.load(open(parent_path))
    fmt = lambda t: " ".join("%.1f" % q for q in t)   # noqa: E731
    lines = ["Pose finder products, one launch each (A) against evaluate + store + multiply through the parent API (B), and against the launch each derives from (C)",
             "tools/pose_products_probe.py; box %s, session %s; one box, one session; microseconds per launch, median of each round" % (new.get("box"), session), ""]
    for shape in SHAPES:
        if shape not in new or shape not in par:
            continue
        r, q = new[shape], par[shape]
        lines.append("%s (B = %d, m = %d, nnz = %d, nnz_h = %d)" % (shape, r["batch"], r["m"], r["nnz"], r["hnnz"]))
        for k in ("C_eval", "C_eval_hess"):
            lines.append("  %-36s rounds: %s" % (k + " (alone)", fmt(r["rounds"][k])))
        for prod in PRODUCTS:
            a, b, bp = r["rounds"]["A_" + prod], r["B_" + prod], q["B_" + prod]
            c = r["rounds"]["C_eval_hess" if prod == "hvp" else "C_eval"]
            lines.append("  %s" % prod)
            lines.append("    A  (one launch)                  rounds: %s" % fmt(a))
            lines.append("    B  (new build)                   rounds: %s" % fmt(b))
            lines.append("    B  (parent build)                rounds: %s" % fmt(bp))
            for k in sorted(r["rounds"]):
                if k.startswith("B_%s_" % prod):
                    lines.append("      %-30s new: %s   parent: %s" % (k, fmt(r["rounds"][k]), fmt(q["rounds"].get(k, []))))
            lines.append("    A / B(parent) = %.3f,  A / C = %.3f (medians of the rounds);  every A round below every B round: %s;  max |A - B| = %.3e" %
                         (np.median(a) / np.median(bp), np.median(a) / np.median(c), "yes" if max(a) < min(min(b), min(bp)) else "NO", r.get("max_abs_diff_" + prod, float("nan"))))
        for k in ("B_eval", "B_eval_hess"):
            lines.append("  %-36s new: %s   parent: %s" % (k, fmt(r["rounds"][k]), fmt(q["rounds"][k])))
        lines.append("")
    text = "\n".join(lines)
    open(out_path, "w").write(text)
    print(text)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lib", help="libhipnlp.so to bind")
    ap.add_argument("--what", default="A,B,C")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--json")
    ap.add_argument("--summarize", nargs=2, metavar=("NEW_JSON", "PARENT_JSON"))
    ap.add_argument("--out")
    ap.add_argument("--session", default=time.strftime("%Y-%m-%d"))
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize[0], a.summarize[1], a.out, a.session)
        return
    what = set(a.what.split(","))
    rec = {"box": socket.gethostname(), "session": a.session}
    for shape in a.shapes.split(","):
        r = probe(os.path.abspath(a.lib), shape, what, a.rounds, a.launches, a.warmup)
        rec[shape] = r
        print(json.dumps({k: r[k] for k in r if k not in ("rounds", "lib")}), flush=True)
        if a.json:
            json.dump(rec, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
