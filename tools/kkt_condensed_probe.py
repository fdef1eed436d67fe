#!/usr/bin/env python3
"""The condensed block factorisation of the KKT solve (hipnlp_kkt_condensed_factor_device; KKTValues.condensed_preconditioner) on the KKT
systems of synthetic workloads' iterates (nlp.kkt at make_workload(seed=8900), on the stairs with place_on_step_flanks; sigma = 0.8; lam, b
standard normal; dx, dc in U[1, 2], one seed, and the same multiplied by 1e-4 — NOT an interior-point method's diagonals; floor 1e-10).
  (a) the launch, timed with HIP events on an explicit stream, `reps` launches per figure: hipnlp_kkt_block_factor_device and
      hipnlp_kkt_condensed_factor_device.  A round is one fresh process per library — the parent commit's (--parent-lib: its
      hipnlp_kkt_block_factor_device is the baseline) and this one's — the two alternating round by round; whether the ranges overlap;
  (b) one iteration of K.solve(minv=...) with the block and with the condensed preconditioner: `iters` iterations at rtol 0 between two
      HIP events, in this library's rounds (the same kernels: expected equal);
  (c) the inertia of the blocks B_k beside that of H_k + dx_k, and K.solve(rtol=1e-8, maxiter=3000, check_every=16) with the block
      preconditioner, the condensed one and the condensed DIAGONAL alone, at both scales of dx, dc.
Records, not requirements: no threshold is set on any of them."""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = ("planar_100x1", "planar_100x64", "stairs_200x16")
SCALES = (1.0, 1e-4)
FLOOR = 1e-10
DEVICE = "cuda"


def system_of(shape):
    """(nlp, K, b_top, b_bottom, the explicit stream everything was enqueued on) of one shape — tools/kkt_ladder_probe.py's systems"""
    import torch
    from hippopt_amd.autograd import KinodynamicNLP
    from hippopt_amd.kinodyn_settings import periodic_step_settings, stairs_settings
    from hippopt_amd.robot_model import synthetic_ergocub
    from hippopt_amd.synthetic import make_workload, place_on_step_flanks
    model = synthetic_ergocub()
    kind, dims = shape.split("_")
    horizon, B = (int(t) for t in dims.split("x"))
    st = (periodic_step_settings if kind == "planar" else stairs_settings)(horizon, model)
    x, p = make_workload(st, model, batch=B, seed=8900)
    if kind == "stairs":
        place_on_step_flanks(x, st, seed=3)
    dev = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=DEVICE)  # noqa: E731
    work = torch.cuda.Stream()        # (an explicit stream: on torch's default one the library would go to a side stream and back)
    with torch.cuda.stream(work):
        nlp = KinodynamicNLP(st, model, batch=B)
        nlp.set_params(p)
        rng = np.random.RandomState(11)
        lam, dx, dc = rng.standard_normal((B, nlp.m)), rng.uniform(1.0, 2.0, (B, nlp.n)), rng.uniform(1.0, 2.0, (B, nlp.m))
        bt, bb = dev(rng.standard_normal((B, nlp.n))), dev(rng.standard_normal((B, nlp.m)))
        K = nlp.kkt(dev(x), 0.8, dev(lam), dev(dx), dev(dc))
    torch.cuda.synchronize()
    return nlp, K, bt, bb, work


def timed(fn, reps):
    """microseconds per call between two HIP events on the current stream, after one warm-up call"""
    import torch
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / reps


def child(shapes, reps, iters):
    """one round of (a) and (b) in this process, with whatever library HIPNLP_LIB_PATH names: {shape: {leg: microseconds}}"""
    import torch
    out = {}
    for shape in shapes:
        nlp, K, bt, bb, work = system_of(shape)
        eng, N = nlp.engine, (nlp.n - 6) // 189
        nb = eng.kkt_block_bytes()
        with torch.cuda.stream(work):
            f = torch.empty(nb[0] // 8, dtype=torch.float64, device=DEVICE)
            piv = torch.empty(nb[1] // 4, dtype=torch.int32, device=DEVICE)
            e, o = (torch.empty(nb[2] // 8, dtype=torch.float64, device=DEVICE) for _ in range(2))
            inertia, status = torch.empty(nlp.batch * N * 3, dtype=torch.int32, device=DEVICE), torch.empty(nlp.batch * N, dtype=torch.int32, device=DEVICE)
            top, bottom = torch.empty(nlp.batch * nlp.n, dtype=torch.float64, device=DEVICE), torch.empty(nlp.batch * nlp.m, dtype=torch.float64, device=DEVICE)
            six = [t.data_ptr() for t in (f, piv, e, o, inertia, status)]
            s = work.cuda_stream
            res = {"factor": timed(lambda: eng.kkt_block_factor_device(K.hess.data_ptr(), *six, dx_ptr=K.dx.data_ptr(), floor=FLOOR, stream=s), reps)}
            if hasattr(eng.lib, "hipnlp_kkt_condensed_factor_device"):
                res["condensed factor"] = timed(lambda: eng.kkt_condensed_factor_device(K.hess.data_ptr(), K.jac.data_ptr(), K.dc.data_ptr(), *six, top.data_ptr(), bottom.data_ptr(),
                                                                                        dx_ptr=K.dx.data_ptr(), floor=FLOOR, stream=s), reps)
                for key, pre in (("iteration, block preconditioner", K.block_preconditioner(FLOOR)), ("iteration, condensed preconditioner", K.condensed_preconditioner(FLOOR))):
                    res[key] = timed(lambda: K.solve(bt, bb, rtol=0.0, maxiter=iters, minv=pre, check_every=16), 1) / iters
        out[shape] = res
        del nlp, K, f, piv, e, o
        torch.cuda.empty_cache()
    return out


def rounds_of(shapes, rounds, reps, iters, parent_lib):
    """{shape: {leg: [microseconds per round]}}: one fresh process per (round, library), the libraries alternating"""
    libs = ([("parent", parent_lib)] if parent_lib else []) + [("this", None)]
    got = {s: {} for s in shapes}
    for _ in range(rounds):
        for tag, path in libs:
            env = dict(os.environ)
            if path:
                env["HIPNLP_LIB_PATH"] = path
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--shapes", ",".join(shapes), "--reps", str(reps), "--iters", str(iters)], env=env,
                               stdout=subprocess.PIPE, text=True, timeout=600)
            if r.returncode != 0:
                raise RuntimeError("the timing process of the %s library ended with %d: nothing more is started" % (tag, r.returncode))
            rec = json.loads(r.stdout.strip().splitlines()[-1])
            print(tag, rec, flush=True)
            for s in shapes:
                for leg, us in rec[s].items():
                    got[s].setdefault(("parent commit's " if tag == "parent" else "") + leg, []).append(us)
    return got


def device_record(shape):
    """(c) of one shape, at both scales"""
    import torch
    nlp, K0, bt, bb, work = system_of(shape)
    recs = []
    with torch.cuda.stream(work):
        for scale in SCALES:
            K = K0 if scale == 1.0 else K0.with_diagonals(K0.dx * scale, K0.dc * scale)
            blk, con = K.block_preconditioner(FLOOR), K.condensed_preconditioner(FLOOR)
            torch.cuda.synchronize()
            neg = lambda pre: pre.inertia[:, :, 1].cpu().numpy()  # noqa: E731
            status = con.status.cpu().numpy()
            rec = {"shape": shape, "scale": scale, "batch": nlp.batch, "N": status.shape[1], "n": nlp.n, "m": nlp.m, "status": {int(s): int((status == s).sum()) for s in np.unique(status)},
                   "negative_block": int(neg(blk).sum()), "negative_condensed": int(neg(con).sum()), "knots_not_pd": int((neg(con) + con.inertia[:, :, 2].cpu().numpy() > 0).sum()),
                   "trajectories_all_pd": int(((neg(con) + con.inertia[:, :, 2].cpu().numpy()).sum(axis=1) == 0).sum()), "most_negative_in_one_block": int(neg(con).max()), "solves": {}}
            for key, mv in (("block preconditioner", blk), ("condensed preconditioner", con), ("condensed diagonal alone", (con.top_diagonal, con.bottom))):
                t0 = time.time()
                z = K.solve(bt, bb, rtol=1e-8, maxiter=3000, minv=mv, check_every=16)
                torch.cuda.synchronize()
                st, its, res = z.status.cpu().numpy(), z.iterations.cpu().numpy(), z.residual.cpu().numpy()
                rec["solves"][key] = {"seconds": time.time() - t0, "status": {int(s): int((st == s).sum()) for s in np.unique(st)},
                                      "iterations": [int(its.min()), int(np.median(its)), int(its.max())], "residual": [float(res.min()), float(np.median(res)), float(res.max())]}
            recs.append(rec)
    return recs


def report(timings, records, session, rounds, reps, iters, parent_lib):
    lines = ["The condensed block factorisation of the KKT solve (tools/kkt_condensed_probe.py); box %s, session %s; one box, one session" % (socket.gethostname(), session), "",
             "KKT systems of synthetic workloads' iterates; sigma = 0.8, lam and b standard normal, dx and dc in U[1, 2] (NOT an interior-point method's) and the same x 1e-4, one seed;",
             "floor %g.  Records, not requirements." % FLOOR, ""]
    fmt = lambda ts: " ".join("%.1f" % t for t in ts)  # noqa: E731
    if timings:
        lines += ["(a), (b) microseconds: HIP events on one explicit stream; a launch: %d launches per figure after one warm-up; an iteration: one K.solve of %d iterations at rtol 0" % (reps, iters),
                  "    (check_every 16) after one warm-up solve, divided by %d.  %d rounds, each a fresh process per library, the parent commit's library (%s) and this one's" % (iters, rounds, "given" if parent_lib else "NOT given: no baseline"),
                  "    alternating round by round.  median [min .. max] and the rounds.", ""]
        for shape, legs in timings.items():
            lines.append("  %s" % shape)
            base = legs.get("parent commit's factor")
            for leg, ts in legs.items():
                med = float(np.median(ts))
                note = ""
                if base and leg in ("factor", "condensed factor"):
                    overlap = min(ts) <= max(base) and min(base) <= max(ts)
                    note = "   = %.3f x the parent's factor launch; the ranges %s" % (med / float(np.median(base)), "overlap" if overlap else "do NOT overlap")
                lines.append("      %-38s median %10.1f  [%.1f .. %.1f]   rounds: %s%s" % (leg, med, min(ts), max(ts), fmt(ts), note))
            if "iteration, block preconditioner" in legs:
                a, b = legs["iteration, block preconditioner"], legs["iteration, condensed preconditioner"]
                lines.append("      an iteration with the condensed preconditioner = %.3f x one with the block preconditioner; the ranges %s"
                             % (float(np.median(b)) / float(np.median(a)), "overlap" if min(a) <= max(b) and min(b) <= max(a) else "do NOT overlap"))
            lines.append("")
    for r in records:
        lines.append("(c) %s, dx and dc x %g (N = %d, B = %d, n = %d, m = %d): knots by status %s" % (r["shape"], r["scale"], r["N"], r["batch"], r["n"], r["m"], r["status"]))
        lines.append("      negative eigenvalues in all blocks: %d of H_k + dx_k, %d of B_k (at most %d in one); knots whose B_k is not positive definite: %d of %d; trajectories with every B_k"
                     % (r["negative_block"], r["negative_condensed"], r["most_negative_in_one_block"], r["knots_not_pd"], r["N"] * r["batch"]))
        lines.append("      positive definite (which proves nothing about K): %d of %d" % (r["trajectories_all_pd"], r["batch"]))
        lines.append("      K.solve(rtol=1e-8, maxiter=3000, check_every=16); status: {status: trajectories}; iterations and residual: min / median / max over the batch")
        for key, s in r["solves"].items():
            lines.append("      %-28s status %-16s iterations %4d / %4d / %4d   residual %.2e / %.2e / %.2e   (%.1f s)" % ((key, str(s["status"])) + tuple(s["iterations"]) + tuple(s["residual"]) + (s["seconds"],)))
        conv = {key: sum(n for st, n in s["status"].items() if st == 0) for key, s in r["solves"].items()}
        lines.append("      converged: %s" % ("NOTHING at this shape and scale: status 1 everywhere" if not any(conv.values()) else ", ".join("%s %d of %d" % (k, v, r["batch"]) for k, v in conv.items())))
        lines.append("")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=96)
    ap.add_argument("--parent-lib", help="the parent commit's libhipnlp.so: the baseline of (a)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_kkt_condensed.txt"))
    ap.add_argument("--session", default=time.strftime("%Y-%m-%d %H:%M:%S"))
    a = ap.parse_args()
    shapes = [s for s in a.shapes.split(",") if s]
    if a.child:
        print(json.dumps(child(shapes, a.reps, a.iters)))
        return
    timings = rounds_of(shapes, a.rounds, a.reps, a.iters, a.parent_lib)     # (the timing processes first: this one has not opened the device yet)
    print(timings, flush=True)
    records = []
    for shape in shapes:
        records += device_record(shape)
        print(records[-2:], flush=True)
    text = report(timings, records, a.session, a.rounds, a.reps, a.iters, a.parent_lib)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
