#!/usr/bin/env python3
"""The per-knot inertia-correcting ladder of the block factorisation (hipnlp_kkt_block_ladder_device; KKTValues.convexify) on the KKT systems
of synthetic workloads' iterates (nlp.kkt at make_workload(seed=8900), on the stairs with place_on_step_flanks; sigma = 0.8; lam, b standard
normal; dx, dc in U[1, 2], one seed — NOT an interior-point method's diagonals; delta_init 1e-4, kappa 8, max_tries 16, floor 1e-10).
  (a) the launch, timed with HIP events on an explicit stream, `reps` launches per figure: hipnlp_kkt_block_factor_device, the ladder
      with max_tries = 0 (the same work) and the ladder with the tries the value runs take.  A round is one fresh process per library —
      the parent commit's (--parent-lib: its hipnlp_kkt_block_factor_device is the baseline) and this one's — the two alternating round
      by round;
  (b) the distribution of tries and of delta per knot, and the statuses;
  (c) K.solve(rtol=1e-8, maxiter=3000, check_every=50): the ladder's preconditioner on the convexified system, the un-laddered block
      preconditioner (|D|) on the same convexified system, and the un-laddered one on the original system;
  (d) --emulation: (b) and (c) at N = 4 with the CPU emulation of these launches (tests/kkt_ladder_emu), the systems of the tests.
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
FLOOR, DELTA_INIT, KAPPA, MAX_TRIES = 1e-10, 1e-4, 8.0, 16
DEVICE = "cuda"


def system_of(shape):
    """(nlp, K, b_top, b_bottom, the explicit stream everything was enqueued on) of one shape"""
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


def child(shapes, reps):
    """one round of (a) in this process, with whatever library HIPNLP_LIB_PATH names: {shape: {leg: microseconds per launch}}"""
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
            delta, tries = torch.empty(nlp.batch * N, dtype=torch.float64, device=DEVICE), torch.empty(nlp.batch * N, dtype=torch.int32, device=DEVICE)
            six = [t.data_ptr() for t in (f, piv, e, o, inertia, status)]
            s = work.cuda_stream
            legs = {"factor": lambda: eng.kkt_block_factor_device(K.hess.data_ptr(), *six, dx_ptr=K.dx.data_ptr(), floor=FLOOR, stream=s)}
            if hasattr(eng.lib, "hipnlp_kkt_block_ladder_device"):
                ladder = lambda mt: eng.kkt_block_ladder_device(K.hess.data_ptr(), *six, delta.data_ptr(), tries.data_ptr(), dx_ptr=K.dx.data_ptr(), floor=FLOOR,  # noqa: E731
                                                                delta_init=DELTA_INIT, kappa=KAPPA, max_tries=mt, stream=s)
                legs["ladder, max_tries = 0"] = lambda: ladder(0)
                legs["ladder, max_tries = 16"] = lambda: ladder(MAX_TRIES)
            res = {}
            for name, fn in legs.items():
                fn()                          # warm-up: tables, code objects
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                res[name] = e0.elapsed_time(e1) * 1000.0 / reps
            if "ladder, max_tries = 16" in res:
                res["slowest knot's tries"] = int(tries.max())
        out[shape] = res
        del nlp, K, f, piv, e, o
        torch.cuda.empty_cache()
    return out


def rounds_of(shapes, rounds, reps, parent_lib):
    """{shape: {"parent factor" / leg: [microseconds per round]}}: one fresh process per (round, library), the libraries alternating"""
    libs = ([("parent", parent_lib)] if parent_lib else []) + [("this", None)]
    got = {s: {} for s in shapes}
    for _ in range(rounds):
        for tag, path in libs:
            env = dict(os.environ)
            if path:
                env["HIPNLP_LIB_PATH"] = path
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--shapes", ",".join(shapes), "--reps", str(reps)], env=env, stdout=subprocess.PIPE, text=True,
                               timeout=900)
            if r.returncode != 0:
                raise RuntimeError("the timing process of the %s library ended with %d: nothing more is started" % (tag, r.returncode))
            rec = json.loads(r.stdout.strip().splitlines()[-1])
            print(tag, rec, flush=True)
            for s in shapes:
                for leg, us in rec[s].items():
                    got[s].setdefault(("parent commit's " if tag == "parent" else "") + leg, []).append(us)
    return got


def device_record(shape):
    """(b) and (c) of one shape"""
    import torch
    nlp, K, bt, bb, work = system_of(shape)
    with torch.cuda.stream(work):
        pre = K.convexify(DELTA_INIT, KAPPA, MAX_TRIES, FLOOR)
        plain_convex = pre.values.block_preconditioner(FLOOR)
        plain = K.block_preconditioner(FLOOR)
        torch.cuda.synchronize()
        tries, delta, status = pre.tries.cpu().numpy(), pre.delta.cpu().numpy(), pre.status.cpu().numpy()
        rec = {"shape": shape, "batch": nlp.batch, "N": tries.shape[1], "n": nlp.n, "m": nlp.m, "max_hess": float(K.hess.abs().max()),
               "tries": {int(t): int((tries == t).sum()) for t in np.unique(tries)}, "status": {int(s): int((status == s).sum()) for s in np.unique(status)},
               "delta": [float(v) for v in (delta.min(), np.median(delta), delta.max())], "quasi_definite": int(pre.quasi_definite.sum()),
               "negative_before": int(plain.inertia[:, :, 1].sum()), "negative_after": int(pre.inertia[:, :, 1].sum()),
               "negative_plain_convex": int(plain_convex.inertia[:, :, 1].sum()), "solves": {}}
        for key, op, mv in (("ladder's factor on the convexified system", pre.values, pre), ("un-laddered |D| on the convexified system", pre.values, plain_convex),
                            ("un-laddered |D| on the original system", K, plain)):
            t0 = time.time()
            z = op.solve(bt, bb, rtol=1e-8, maxiter=3000, minv=mv, check_every=50)
            torch.cuda.synchronize()
            st, its, res = z.status.cpu().numpy(), z.iterations.cpu().numpy(), z.residual.cpu().numpy()
            rec["solves"][key] = {"seconds": time.time() - t0, "status": {int(s): int((st == s).sum()) for s in np.unique(st)},
                                  "iterations": [int(its.min()), int(np.median(its)), int(its.max())], "residual": [float(res.min()), float(np.median(res)), float(res.max())]}
    return rec


def emulation_records():
    """(d): the real N = 4 systems of tests/test_kkt_ladder_hostemu.py with the CPU emulation"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import kkt_check
    from hippopt_amd.robot_model import synthetic_ergocub
    from kkt_ladder_emu_lib import KktLadderEmu
    from test_kkt_block_hostemu import real_runs
    from test_lagrangian_grad_hostemu import MAKERS
    model, out = synthetic_ergocub(), []
    for name in ("stairs", "periodic"):
        _, pat, d = real_runs(model, name, 4)
        emu = KktLadderEmu(MAKERS[name](4, model), model)
        lad = emu.block_ladder(d["hess"], d["dx"], FLOOR, DELTA_INIT, KAPPA, MAX_TRIES)
        dxp = emu.convexified_dx(d["dx"], lad.delta)
        b = np.concatenate([d["bt"], d["bb"]])
        rec = {"name": name, "tries": lad.tries.tolist(), "delta": lad.delta.tolist(), "status": lad.status.tolist(), "solves": {}}
        for key, dx, blk in (("ladder's factor on the convexified system", dxp, lad), ("un-laddered |D| on the convexified system", dxp, emu.block_factor(d["hess"], dxp, FLOOR)),
                             ("un-laddered |D| on the original system", d["dx"], emu.block_factor(d["hess"], d["dx"], FLOOR))):
            diag = emu.diagonal_preconditioner(d["hess"], d["jac"], dx, d["dc"], FLOOR)
            s = emu.block_solve(d["hess"], d["jac"], d["bt"], d["bb"], blk, (diag.top, diag.bottom), dx=dx, dc=d["dc"], rtol=1e-8, maxiter=3000)
            K = kkt_check.dense(emu.n, emu.m, *pat[:2], d["hess"], *pat[2:], d["jac"], dx, d["dc"])
            true = float(np.linalg.norm(K @ np.concatenate([s.top, s.bottom]) - b) / np.linalg.norm(b))
            rec["solves"][key] = (s.status, s.iterations, s.residual, true)
        out.append(rec)
    return out


def report(timings, records, emulated, session, rounds, reps, parent_lib):
    lines = ["The per-knot inertia-correcting ladder of the block factorisation (tools/kkt_ladder_probe.py); box %s, session %s; one box, one session" % (socket.gethostname(), session), "",
             "KKT systems of synthetic workloads' iterates; sigma = 0.8, lam and b standard normal, dx and dc in U[1, 2] (NOT an interior-point method's), one seed.",
             "delta_init %g, kappa %g, max_tries %d (IPOPT's first_hessian_perturbation and perturb_inc_fact, untuned here), floor %g." % (DELTA_INIT, KAPPA, MAX_TRIES, FLOOR),
             "Records, not requirements.", ""]
    fmt = lambda ts: " ".join("%.1f" % t for t in ts)  # noqa: E731
    if timings:
        lines += ["(a) microseconds per launch: HIP events on one explicit stream, %d launches per figure after one warm-up; %d rounds, each a fresh process per library, the parent" % (reps, rounds),
                  "    commit's library (%s) and this one's alternating round by round.  median [min .. max] and the rounds." % ("given" if parent_lib else "NOT given: no baseline"), ""]
        for shape, legs in timings.items():
            lines.append("  %s" % shape)
            base = None
            for leg, ts in legs.items():
                if leg == "slowest knot's tries":
                    lines.append("      the slowest knot of the launch took %d tries" % ts[0])
                    continue
                med = float(np.median(ts))
                if leg.startswith("parent") and leg.endswith("factor"):
                    base = med
                lines.append("      %-34s median %10.1f  [%.1f .. %.1f]   rounds: %s%s" % (leg, med, min(ts), max(ts), fmt(ts), ("   = %.2f x the parent's factor launch" % (med / base)) if base and not leg.startswith("parent") else ""))
            lines.append("")
    for r in records:
        lines.append("(b) %s (N = %d, B = %d, n = %d, m = %d; max |H| %.2e): knots by status %s; by tries %s" % (r["shape"], r["N"], r["batch"], r["n"], r["m"], r["max_hess"], r["status"], r["tries"]))
        lines.append("      delta per knot min / median / max: %.3e / %.3e / %.3e; negative eigenvalues in all blocks: %d before, %d after (un-laddered factor of the convexified blocks: %d);"
                     % (tuple(r["delta"]) + (r["negative_before"], r["negative_after"], r["negative_plain_convex"])))
        lines.append("      trajectories with .quasi_definite: %d of %d" % (r["quasi_definite"], r["batch"]))
        lines.append("(c) K.solve(rtol=1e-8, maxiter=3000, check_every=50); status: {status: trajectories}; iterations and residual: min / median / max over the batch")
        for key, s in r["solves"].items():
            lines.append("      %-44s status %-14s iterations %4d / %4d / %4d   residual %.2e / %.2e / %.2e   (%.1f s)" % ((key, str(s["status"])) + tuple(s["iterations"]) + tuple(s["residual"]) + (s["seconds"],)))
        conv = sum(n for st, n in r["solves"]["ladder's factor on the convexified system"]["status"].items() if st == 0)
        lines.append("      %s" % ("NO trajectory converged on the convexified system at this shape." if conv == 0 else "%d of %d trajectories converged on the convexified system." % (conv, r["batch"])))
        lines.append("")
    if emulated:
        lines.append("(d) the CPU emulation of these launches on the real N = 4 systems of tests/test_kkt_ladder_hostemu.py (rtol 1e-8, maxiter 3000): status, iterations, residual, TRUE relative residual")
        for r in emulated:
            lines.append("  %s N = 4: tries %s, delta %s, status %s" % (r["name"], r["tries"], ["%.3e" % v for v in r["delta"]], r["status"]))
            for key, s in r["solves"].items():
                lines.append("      %-44s status %d after %4d iterations, residual %.3e, true %.3e" % ((key,) + tuple(s)))
        lines.append("")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", help="the parent commit's libhipnlp.so: the baseline of (a)")
    ap.add_argument("--no-device", action="store_true", help="leave (a), (b) and (c) out")
    ap.add_argument("--emulation", action="store_true", help="add (d)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_kkt_ladder.txt"))
    ap.add_argument("--session", default=time.strftime("%Y-%m-%d %H:%M:%S"))
    a = ap.parse_args()
    shapes = [s for s in a.shapes.split(",") if s]
    if a.child:
        print(json.dumps(child(shapes, a.reps)))
        return
    timings, records = {}, []
    if not a.no_device:
        timings = rounds_of(shapes, a.rounds, a.reps, a.parent_lib)     # (the timing processes first: this one has not opened the device yet)
        print(timings, flush=True)
        for shape in shapes:
            records.append(device_record(shape))
            print(records[-1], flush=True)
    emulated = emulation_records() if a.emulation else []
    text = report(timings, records, emulated, a.session, a.rounds, a.reps, a.parent_lib)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
