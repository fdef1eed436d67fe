#!/usr/bin/env python3
"""Hessian-vector product y = H(x, sigma, lambda) v of a batch: the one launch (A, hipnlp_eval_hess_vec_device) against "evaluate, store,
multiply" through the API of a build WITHOUT it (B), timed with HIP events (torch.cuda.Event), one event between consecutive launches.

    B = hipnlp_eval_hess_device into HBM
      + min(two torch.sparse CSR mat-vecs, block diagonal over the batch: the upper triangle with the diagonal (the handle's (column, row)
            order IS its CSR order: the values are used where they are) and the strict lower triangle (values gathered into row order),
            an index_add_ over the triplets, rows and columns (no order needed))
    C = hipnlp_eval_hess_device alone            (reported beside A, not gated)
    D = hipnlp_hess_times_device alone           (reported against the bytes it must move, not gated)

Every quantity is timed in `--rounds` rounds of `--launches` launches after a warm-up, the legs alternating within a round; a round's
figure is the median of its launches (microseconds).  B uses only entry points that a build of the parent commit has, so the same
script can run it on that build; processes of the two builds alternate round by round (--rounds 1 --append), so that a drift of the
box over the job reaches both alike:

    for r in 1 2 3 4 5; do
        python tools/hessian_vector_probe.py --lib NEW.so    --what A,B,C,D --rounds 1 --append --json new.json
        python tools/hessian_vector_probe.py --lib PARENT.so --what B       --rounds 1 --append --json parent.json
    done
    python tools/hessian_vector_probe.py --summarize new.json parent.json --out report.txt

Gates (--summarize): every round median of A below every round median of B (new build), and the median of B's round medians on the new
build within the round-to-round spread (max - min of the round medians) of B on the parent build, widened by the new build's own spread."""
import argparse
import json
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
    """per-launch microseconds of `count` consecutive calls of fn, an event between every two"""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(count + 1)]
    ev[0].record()
    for i in range(count):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    return np.array([ev[i].elapsed_time(ev[i + 1]) * 1000.0 for i in range(count)])


def probe(lib_path, shape, what, rounds, launches, warmup):
    # (every launch and every event on one explicit stream: a NULL stream would be each handle's own to the library)
    import torch
    work = torch.cuda.Stream()
    with torch.cuda.stream(work):
        return probe_on(lib_path, shape, what, rounds, launches, warmup, work.cuda_stream)


def probe_on(lib_path, shape, what, rounds, launches, warmup, stream):
    import torch
    from hippopt_amd import hipnlp
    from hippopt_amd.robot_model import synthetic_ergocub
    hipnlp._LIB_PATH = lib_path                     # (this process binds the library under test and no other)
    model = synthetic_ergocub()
    st, x, p = make_shape(shape, model)
    B = x.shape[0]
    eng = hipnlp.HipNlp(st, model, batch=B, jac_varying_first=True, library=lib_path)   # (the shapes of the gate: varying-first handles)
    eng.set_params(p)
    n, m, nnz = eng.n, eng.m, eng.hess_nnz()
    dev = "cuda"
    xd = torch.tensor(x, device=dev)
    rng = np.random.RandomState(7)
    sig = torch.tensor(rng.uniform(0.5, 1.5, B), device=dev)
    lam = torch.tensor(rng.standard_normal((B, m)), device=dev)
    v = torch.tensor(rng.standard_normal((B, n)), device=dev)
    vals = torch.zeros((B, nnz), dtype=torch.float64, device=dev)
    out = torch.zeros((B, n), dtype=torch.float64, device=dev)
    ir, jc = eng.hess_sparsity()
    ir, jc = ir.astype(np.int64), jc.astype(np.int64)
    # upper triangle with the diagonal = the transposed triplets: rows jc, columns ir; strict lower triangle: rows ir, columns jc
    itype = torch.int32 if B * nnz < 2 ** 31 else torch.int64
    offs = torch.arange(B, device=dev, dtype=torch.int64)[:, None] * n

    def csr(rows, cols, keep):
        order = np.lexsort((cols[keep], rows[keep]))
        sel = np.flatnonzero(keep)[order]
        counts = torch.tensor(np.bincount(rows[sel], minlength=n), device=dev)
        crow = torch.zeros(B * n + 1, dtype=torch.int64, device=dev)
        crow[1:] = torch.cumsum(counts.repeat(B), 0)
        col = (offs + torch.tensor(cols[sel], device=dev)[None, :]).reshape(-1)
        ident = sel.size == nnz and bool(np.array_equal(sel, np.arange(nnz)))
        return crow.to(itype), col.to(itype), None if ident else torch.tensor(sel, device=dev)
    up = csr(jc, ir, np.ones(nnz, bool))
    lo = csr(ir, jc, ir != jc)
    ir_t, jc_t = torch.tensor(ir, device=dev), torch.tensor(jc, device=dev)
    off_t = torch.tensor(np.flatnonzero(ir != jc), device=dev)
    ir_o, jc_o = ir_t[off_t], jc_t[off_t]
    vcol = v.reshape(-1, 1)

    def eval_hess():
        eng.eval_hess_device(xd.data_ptr(), sig.data_ptr(), lam.data_ptr(), vals.data_ptr(), stream=stream)

    def prod_csr():
        y = None
        for crow, col, sel in (up, lo):
            a = torch.sparse_csr_tensor(crow, col, (vals if sel is None else vals[:, sel]).reshape(-1), (B * n, B * n))
            t = torch.sparse.mm(a, vcol)
            y = t if y is None else y + t
        out.copy_(y.reshape(B, n))

    def prod_index_add():
        y = torch.zeros((B, n), dtype=torch.float64, device=dev)
        y.index_add_(1, ir_t, vals * v[:, jc_t])
        y.index_add_(1, jc_o, vals[:, off_t] * v[:, ir_o])
        out.copy_(y)

    def fused():
        eng.eval_hess_vec_device(xd.data_ptr(), sig.data_ptr(), lam.data_ptr(), v.data_ptr(), out.data_ptr(), stream=stream)

    def times():
        eng.hess_times_device(vals.data_ptr(), v.data_ptr(), out.data_ptr(), stream=stream)

    parts = {}
    if "B" in what:
        parts.update({"B_eval_hess": eval_hess, "B_prod_csr": prod_csr, "B_prod_index_add": prod_index_add})
    if "A" in what:
        parts["A"] = fused
    if "C" in what:
        parts["C"] = eval_hess
    if "D" in what:
        parts["D"] = times
    for name in list(parts):   # warm-up; a product that this torch build cannot run is left out and said so
        try:
            eval_hess()
            for _ in range(warmup):
                parts[name]()
            torch.cuda.synchronize()
        except RuntimeError as err:
            if not name.startswith("B_prod"):
                raise
            print("%s: %s: %s" % (shape, name, err), file=sys.stderr)
            del parts[name]
    res = {k: [] for k in parts}
    # rounds: A's launches, then B's parts (the products read the values of a fresh evaluation), then C and D, alternating
    for _ in range(rounds):
        for name in (["A"] if "A" in parts else []) + [k for k in parts if k.startswith("B")] + [k for k in ("C", "D") if k in parts]:
            eval_hess()
            res[name].append(float(np.median(event_times(torch, parts[name], launches))))
    out_rec = {"shape": shape, "batch": B, "n": n, "m": m, "nnz": nnz, "N": st.horizon_length, "lib": lib_path, "rounds": res}
    if "B" in what:
        pr = [min(t) for t in zip(*[res[k] for k in res if k.startswith("B_prod")])]
        out_rec["B"] = [a + b for a, b in zip(res["B_eval_hess"], pr)]
    for k in ("A", "C", "D"):
        if k in what:
            out_rec[k] = res[k]
    if "A" in what and "B" in what:   # the vectors themselves agree
        torch.cuda.synchronize()
        eval_hess()
        prod_index_add()
        ref = out.clone()
        fused()
        torch.cuda.synchronize()
        out_rec["max_abs_diff_A_vs_B"] = float((out - ref).abs().max())
        a1 = out.clone()
        times()
        torch.cuda.synchronize()
        out_rec["A_equals_D_bitwise"] = bool(torch.equal(a1.view(torch.int64), out.view(torch.int64)))
    return out_rec


def summarize(new_path, parent_path, out_path, session):
    new, par = json.load(open(new_path)), json.load(open(parent_path))
    lines = ["Hessian-vector product H(x, sigma, lambda) v: one launch (A) against evaluate + store + multiply through the parent API (B)",
             "tools/hessian_vector_probe.py; box %s, session %s; one box, one session; microseconds per launch, median of each round" % (new.get("box"), session), ""]
    ok = True
    for shape in SHAPES:
        if shape not in new or shape not in par:
            continue
        r = new[shape]
        a, b, c, d = r["A"], r["B"], r["C"], r["D"]
        bp = par[shape]["B"]
        gate_ab = max(a) < min(b)
        spread = max(max(bp) - min(bp), max(b) - min(b))
        gate_reg = abs(float(np.median(b)) - float(np.median(bp))) <= spread
        ok &= gate_ab and gate_reg
        nnz_knot = r["nnz"] // r["N"]
        floor_us = 8.0 * (nnz_knot + 2 * 189) * r["N"] * r["batch"] / 8e12 * 1e6
        lines.append("%s (B = %d, n = %d, nnz_h = %d)" % (shape, r["batch"], r["n"], r["nnz"]))
        lines.append("  A  (fused launch)               rounds: %s" % " ".join("%.1f" % t for t in a))
        lines.append("  B  (new build)                  rounds: %s" % " ".join("%.1f" % t for t in b))
        lines.append("  B  (parent build)               rounds: %s" % " ".join("%.1f" % t for t in bp))
        for k in sorted(r["rounds"]):
            if k.startswith("B_"):
                lines.append("    %-28s new: %s   parent: %s" % (k, " ".join("%.1f" % t for t in r["rounds"][k]),
                                                                  " ".join("%.1f" % t for t in par[shape]["rounds"].get(k, []))))
        lines.append("  C  (eval_hess_device alone)     rounds: %s" % " ".join("%.1f" % t for t in c))
        lines.append("  D  (hess_times_device alone)    rounds: %s" % " ".join("%.1f" % t for t in d))
        lines.append("  A / B = %.3f,  A / C = %.3f (medians of the rounds; spread of C %.1f)" % (np.median(a) / np.median(b), np.median(a) / np.median(c), max(c) - min(c)))
        lines.append("  D = %.1f against %.1f for 8 (nnz_knot + 2 x 189) bytes per knot at 8 TB/s: %.1f x" % (np.median(d), floor_us, np.median(d) / floor_us))
        lines.append("  gate: every A round below every B round: %s;  B new %.1f vs parent %.1f within spread %.1f: %s" %
                     ("yes" if gate_ab else "NO", np.median(b), np.median(bp), spread, "yes" if gate_reg else "NO"))
        lines.append("  max |A - B| over the batch: %.3e;  A == D bitwise: %s" % (r.get("max_abs_diff_A_vs_B", float("nan")), r.get("A_equals_D_bitwise")))
        lines.append("")
    lines.append("ALL GATES PASS" if ok else "A GATE FAILED")
    text = "\n".join(lines) + "\n"
    open(out_path, "w").write(text)
    print(text)
    return ok


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lib", help="libhipnlp.so to bind")
    ap.add_argument("--what", default="A,B,C,D")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--json")
    ap.add_argument("--append", action="store_true", help="add this process's rounds to those already in --json")
    ap.add_argument("--summarize", nargs=2, metavar=("NEW_JSON", "PARENT_JSON"))
    ap.add_argument("--out")
    ap.add_argument("--session", default=time.strftime("%Y-%m-%d %H:%M:%S"))
    a = ap.parse_args()
    if a.summarize:
        sys.exit(0 if summarize(a.summarize[0], a.summarize[1], a.out, a.session) else 1)
    what = set(a.what.split(","))
    rec = {"box": socket.gethostname(), "session": a.session}
    old = json.load(open(a.json)) if (a.append and a.json and os.path.exists(a.json)) else {}
    for shape in a.shapes.split(","):
        r = probe(os.path.abspath(a.lib), shape, what, a.rounds, a.launches, a.warmup)
        if shape in old:   # (--append: this process's rounds behind those of earlier processes — rounds of two builds interleaved by process)
            for k in ("A", "B", "C", "D"):
                if k in r:
                    r[k] = old[shape][k] + r[k]
            for k in r["rounds"]:
                r["rounds"][k] = old[shape]["rounds"][k] + r["rounds"][k]
        rec[shape] = r
        print(json.dumps({k: r[k] for k in ("shape", "A", "B", "C", "D") if k in r}), flush=True)
    if a.json:
        json.dump(rec, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
