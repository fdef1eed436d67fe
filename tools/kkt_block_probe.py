#!/usr/bin/env python3
"""The block preconditioner of the KKT solve (KKTValues.block_preconditioner: hipnlp_kkt_block_factor_device and the diagonal launch;
KKTValues.solve(minv=it): hipnlp_kkt_minres_block_device) against the diagonal one, on the KKT systems of synthetic workloads' iterates
(nlp.kkt at make_workload(seed=8900), on the stairs with place_on_step_flanks; sigma = 0.8; lam, b standard normal; dx, dc in U[1, 2], one
seed — NOT an interior-point method's diagonals).  Per shape, timed with HIP events on an explicit stream:
  (a) the factor launch: microseconds per K.block_preconditioner() — both of its launches — and beside it the diagonal launch alone,
      the factor launch by difference; a round is `reps` builds per leg, the legs alternating in one process;
  (b) microseconds per MINRES iteration with either preconditioner: K.solve(rtol=0, maxiter=ITERS, check_every=0) — no trajectory can
      stop early, nothing waits for the host — elapsed / ITERS, the two legs alternating round by round;
  (c) iterations, status and final residual of K.solve(rtol=1e-8, maxiter=3000, check_every=50) with both, and the inertia the factor
      launch reported.
Records, not requirements: no threshold is set on any of them."""
import argparse
import os
import socket
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = ("planar_100x1", "planar_100x64", "stairs_200x16")
FLOOR = 1e-10
ITERS = 100
DEVICE = "cuda"


def settings_of(name, model):
    from hippopt_amd.kinodyn_settings import periodic_step_settings, stairs_settings
    kind, dims = name.split("_")
    horizon, batch = (int(t) for t in dims.split("x"))
    return (periodic_step_settings if kind == "planar" else stairs_settings)(horizon, model), batch


def probe(shape, rounds, reps):
    import torch
    from hippopt_amd.autograd import KinodynamicNLP
    from hippopt_amd.robot_model import synthetic_ergocub
    from hippopt_amd.synthetic import make_workload, place_on_step_flanks
    model = synthetic_ergocub()
    st, B = settings_of(shape, model)
    x, p = make_workload(st, model, batch=B, seed=8900)
    if shape.startswith("stairs"):
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

        def timed(fn, count):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(count):
                out = fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1000.0 / count, out

        # (a) the builds
        legs = {"block": lambda: K.block_preconditioner(FLOOR), "diagonal": lambda: K.diagonal_preconditioner(FLOOR)}
        build = {k: [] for k in legs}
        for fn in legs.values():
            timed(fn, 1)                 # warm-up: allocator, tables, code objects
        for _ in range(rounds):
            for k, fn in legs.items():
                build[k].append(timed(fn, reps)[0])
        M, diag = K.block_preconditioner(FLOOR), K.diagonal_preconditioner(FLOOR)
        torch.cuda.synchronize()
        inertia, fstatus = M.inertia.cpu().numpy(), M.status.cpu().numpy()
        # (b) microseconds per iteration
        per = {"block": [], "diagonal": []}
        run = {"block": lambda: K.solve(bt, bb, rtol=0.0, maxiter=ITERS, minv=M, check_every=0), "diagonal": lambda: K.solve(bt, bb, rtol=0.0, maxiter=ITERS, minv=diag, check_every=0)}
        ran = {}
        for k, fn in run.items():
            timed(fn, 1)
        for _ in range(rounds):
            for k, fn in run.items():
                t, z = timed(fn, 1)
                per[k].append(t / ITERS)
                ran[k] = (int(z.iterations.min()), int(z.iterations.max()))
        # (c) to rtol 1e-8
        solves = {}
        for k, mv in (("block", M), ("diagonal", diag)):
            t0 = time.time()
            z = K.solve(bt, bb, rtol=1e-8, maxiter=3000, minv=mv, check_every=50)
            torch.cuda.synchronize()
            status, its, res = z.status.cpu().numpy(), z.iterations.cpu().numpy(), z.residual.cpu().numpy()
            solves[k] = {"seconds": time.time() - t0, "status": {int(s): int((status == s).sum()) for s in np.unique(status)},
                         "iterations": (int(its.min()), int(np.median(its)), int(its.max())), "residual": (float(res.min()), float(np.median(res)), float(res.max()))}
        return {"shape": shape, "batch": B, "N": st.horizon_length, "n": nlp.n, "m": nlp.m, "reps": reps, "build": build, "per_iteration": per, "ran": ran, "solves": solves,
                "max_hess": float(K.hess.abs().max()), "negative": (int(inertia[:, :, 1].min()), int(inertia[:, :, 1].max())), "zero": int(inertia[:, :, 2].sum()),
                "factor_status": {int(s): int((fstatus == s).sum()) for s in np.unique(fstatus)}, "factor_bytes": int(nlp.engine.kkt_block_bytes()[0])}


def report(records, session):
    lines = ["The block preconditioner of the KKT solve against the diagonal one (tools/kkt_block_probe.py); box %s, session %s; one box, one session" % (socket.gethostname(), session), "",
             "KKT systems of synthetic workloads' iterates; sigma = 0.8, lam and b standard normal, dx and dc in U[1, 2] (NOT an interior-point method's), one seed; floor %g." % FLOOR,
             "Records, not requirements.  microseconds: HIP events on one stream; a round's figure is elapsed / count; the legs alternate round by round in one process.", ""]
    fmt = lambda ts: " ".join("%.1f" % t for t in ts)  # noqa: E731
    for r in records:
        lines.append("%s (N = %d, B = %d, n = %d, m = %d; max |H| %.2e; stored factor %.1f MB; knot blocks with status %s; negative eigenvalues per block %d .. %d, zero pivots %d)"
                     % (r["shape"], r["N"], r["batch"], r["n"], r["m"], r["max_hess"], r["factor_bytes"] / 1e6, r["factor_status"], r["negative"][0], r["negative"][1], r["zero"]))
        b, p = r["build"], r["per_iteration"]
        mb, md = float(np.median(b["block"])), float(np.median(b["diagonal"]))
        lines.append("  (a) build, us (%d per round)   block (factor launch + diagonal launch) median %9.1f   rounds: %s" % (r["reps"], mb, fmt(b["block"])))
        lines.append("                                  diagonal launch alone                  median %9.1f   rounds: %s" % (md, fmt(b["diagonal"])))
        lines.append("                                  the factor launch, by difference of the medians: %.1f us" % (mb - md))
        pb, pd = float(np.median(p["block"])), float(np.median(p["diagonal"]))
        lines.append("  (b) us per iteration (%d iterations per round, rtol 0; iterations run: block %s, diagonal %s)" % (ITERS, r["ran"]["block"], r["ran"]["diagonal"]))
        lines.append("                                  block    median %8.1f   rounds: %s" % (pb, fmt(p["block"])))
        lines.append("                                  diagonal median %8.1f   rounds: %s" % (pd, fmt(p["diagonal"])))
        lines.append("                                  block / diagonal = %.2f (medians): an iteration with the block preconditioner is %s" % (pb / pd, "SLOWER" if pb > pd else "not slower"))
        lines.append("  (c) K.solve(rtol=1e-8, maxiter=3000, check_every=50); status: {status: trajectories}; iterations and residual: min / median / max over the batch")
        for key in ("block", "diagonal"):
            s = r["solves"][key]
            lines.append("      %-9s status %-16s iterations %4d / %4d / %4d   residual %.2e / %.2e / %.2e   (%.1f s)" % ((key, str(s["status"])) + s["iterations"] + s["residual"] + (s["seconds"],)))
        lines.append("")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--session", default=time.strftime("%Y-%m-%d %H:%M:%S"))
    a = ap.parse_args()
    records = []
    for shape in [s for s in a.shapes.split(",") if s]:
        records.append(probe(shape, a.rounds, a.reps))
        print(records[-1], flush=True)
    text = report(records, a.session)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
