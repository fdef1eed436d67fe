#!/usr/bin/env python3
"""The dense L D L^T of the pose finder's KKT matrix on the REAL value runs of a batch of poses (PoseNLP.kkt at make_pose_workload iterates;
sigma in U[0.5, 1.5], lam and b standard normal, dx and dc in U[1, 2] — NOT an interior-point method's; the setting of
tools/pose_kkt_probe.py), timed with HIP events (torch.cuda.Event) on one explicit stream, `--rounds` rounds per leg, the legs alternating
in one process; medians and ranges of the rounds, every round printed.

    A    K.solve_direct(b): assemble, factor, inertia and ONE solve.                                  ONE launch per round.
    A'   the inertia-only call (nrhs = 0, no factor stored).                                          ONE launch per round.
    A''  F.solve(b) from the stored factor of K.factor() (the factorisation outside the timing).      ONE launch per round.
    B    K.solve(rtol=1e-8, maxiter=1000, minv="diagonal"): MINRES, every pose to its own convergence. ONE launch per round.
    C    torch.linalg.solve on the dense [batch, n + m, n + m] K in chunks of 256 systems (assembly outside the timing; the launches
         inside a call are not counted).

The condition: every round of A lies below every round of C.  A against B is reported, not required.

In front of the timings the file carries the CPU emulation's table (tests/pose_ldl_emu; no device): for each of the 6 x (3 + 3) systems
of tests/pose_ldl_check.py the normwise backward error eta of the direct solve and of numpy.linalg.solve, the bound, the inertia and the
pivot kinds.

    python tools/pose_ldl_probe.py --out profiles/r15_pose_ldl.txt          (--emulation-only: the table alone, no device)"""
import argparse
import os
import socket
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for q in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if q not in sys.path:
        sys.path.insert(0, q)

SHAPES = ("planar_4096", "planar_16384", "steps_4096", "steps_16384")
DEVICE = "cuda"
CHUNK = 256


def emulation_section():
    import pose_ldl_check as plc
    from hippopt_amd.robot_model import synthetic_ergocub
    from pose_ldl_emu_lib import PoseLdlEmu
    from test_pose_body_hostemu import VARIANTS, variants
    model = synthetic_ergocub()
    lines = ["CPU emulation of the kernels (tests/pose_ldl_emu; the device's bits: tests/test_gpu_pose_ldl.py): eta = |K z - b|_inf / (|K|_inf |z|_inf + |b|_inf) of the",
             "direct solve and of numpy.linalg.solve on the same dense system, the bound max(16 eta_numpy, N 2^-53), the inertia of D (equal to eigvalsh's sign counts in",
             "every case), the smallest |eigenvalue| / |K|_2 of the reference, and the pivots (2x2, 1x1 with an interchange, 1x1 without).", ""]
    for name in VARIANTS:
        e = PoseLdlEmu(variants(model)[name], model)
        ir, jc, hr, hc = e.sparsity()
        pat = (hr, hc, ir, jc)
        for label, d, ref_d in plc.synthetic_systems(e, pat) + [("real %d" % b, d, d) for b, d in enumerate(plc.real_runs(model, name, variants, e))]:
            K, b = plc.dense_of(e, pat, d), plc.rhs_of(d)
            f = e.factor(d["hess"], d["jac"], d["dx"], d["dc"], d["bt"][None], d["bb"][None])
            bound, ref = plc.eta_bound(K, b)
            counts, gap = plc.sign_counts(plc.dense_of(e, pat, ref_d))
            lines.append("  %-12s %-15s N %3d  eta %.3e  numpy %.3e  bound %.3e  status %d  inertia %-14s eigvalsh %-14s gap %.1e  pivots %s"
                         % (name, label, e.N, plc.eta(K, np.concatenate([f.top[0], f.bottom[0]]), b), ref, bound, f.status, f.inertia, counts, gap, plc.pivot_kinds(f.pivots)))
        d = plc.indefinite(plc.synthetic_systems(e, pat)[0][1])
        f = e.factor(d["hess"], d["jac"], d["dx"], d["dc"], delta_init=plc.DELTA_INIT, kappa=plc.KAPPA, max_tries=16)
        lines.append("  %-12s ladder (synthetic 0.05, dx negated; delta_init %g, kappa %g): numpy's walk ends at (try, delta) %s, the emulation at (%d, %r), inertia %s"
                     % (name, plc.DELTA_INIT, plc.KAPPA, plc.numpy_ladder(e, pat, d), f.tries, f.delta, f.inertia))
    return "\n".join(lines) + "\n"


def probe(shape, rounds):
    import torch
    from hippopt_amd.autograd import PoseNLP
    from hippopt_amd.pose_settings import make_pose_workload
    from hippopt_amd.robot_model import synthetic_ergocub
    from pose_kkt_probe import dense_k
    from test_pose_body_hostemu import variants
    model = synthetic_ergocub()
    kind, B = shape.split("_")
    B = int(B)
    st = variants(model)["default" if kind == "planar" else "steps"]
    x64, p64 = make_pose_workload(st, model, 64, 1234)
    cyc = np.arange(B) % 64
    dev = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=DEVICE)  # noqa: E731
    work = torch.cuda.Stream()        # (an explicit stream: on torch's default one the library would go to a side stream and back)
    with torch.cuda.stream(work):
        nlp = PoseNLP(st, model, batch=B)
        nlp.set_params(p64[cyc])
        n, m = nlp.n, nlp.m
        rng = np.random.RandomState(7)
        sig, lam = dev(rng.uniform(0.5, 1.5, B)), dev(rng.standard_normal((B, m)))
        dx, dc = dev(rng.uniform(1.0, 2.0, (B, n))), dev(rng.uniform(1.0, 2.0, (B, m)))
        bt, bb = dev(rng.standard_normal((B, n))), dev(rng.standard_normal((B, m)))
        K = nlp.kkt(dev(x64[cyc]), sig, lam, dx, dc)
        F = K.factor()
        conv = K.solve(bt, bb, rtol=1e-8, maxiter=1000, minv="diagonal")
        inertia = torch.empty((B, 3), dtype=torch.int32, device=DEVICE)
        status = torch.empty((B,), dtype=torch.int32, device=DEVICE)
        s = torch.cuda.current_stream().cuda_stream

        def inertia_only():
            nlp.engine.kkt_ldl_device(K.hess.data_ptr(), K.jac.data_ptr(), inertia.data_ptr(), status.data_ptr(), dx_ptr=dx.data_ptr(), dc_ptr=dc.data_ptr(), stream=s)
            return inertia
        D = dense_k(torch, nlp, K)
        rhs = torch.cat([bt, bb], 1)[:, :, None]
        legs = {"A": lambda: K.solve_direct(bt, bb), "A'": inertia_only, "A''": lambda: F.solve(bt, bb),
                "B": lambda: K.solve(bt, bb, rtol=1e-8, maxiter=1000, minv="diagonal"),
                "C": lambda: torch.cat([torch.linalg.solve(D[i:i + CHUNK], rhs[i:i + CHUNK]) for i in range(0, B, CHUNK)])}

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1000.0, out
        outs = {k: timed(fn)[1] for k, fn in legs.items()}        # warm-up: allocator, code objects, rocSOLVER's handle
        rec = {"shape": shape, "B": B, "n": n, "m": m, "rounds": {k: [] for k in legs}}
        for _ in range(rounds):
            for k, fn in legs.items():
                rec["rounds"][k].append(timed(fn)[0])
        # that the legs compute the same thing
        za = torch.cat(outs["A"][:2], 1)
        zc = outs["C"][:, :, 0]
        scale = zc.abs().amax(1)
        rec["a_c_diff"] = float(((za - zc).abs().amax(1) / scale).max())
        rec["b_c_diff"] = float(((torch.cat([conv.top, conv.bottom], 1) - zc).abs().amax(1) / scale).max())
        rec["a2_equal"] = bool(torch.equal(torch.cat(outs["A''"], 1), za))
        its, st_a = conv.iterations.cpu().numpy(), outs["A"][3].cpu().numpy()
        rec["iterations"] = (int(its.min()), int(np.median(its)), int(its.max()))
        rec["status"] = {int(v): int((st_a == v).sum()) for v in np.unique(st_a)}
        ine = outs["A"][2].cpu().numpy()
        rec["inertia_wanted"] = int(((ine[:, 0] == n) & (ine[:, 1] == m) & (ine[:, 2] == 0)).sum())
        rec["inertia_equal"] = bool(np.array_equal(ine, inertia.cpu().numpy()))
        return rec


def report(recs, session):
    us = lambda ts: " ".join("%.1f" % t for t in ts)  # noqa: E731
    lines = ["The dense L D L^T of the pose finder's KKT matrix, one workgroup of 1 024 threads per pose (tools/pose_ldl_probe.py); box %s, session %s; one box, one session"
             % (socket.gethostname(), session),
             "Real value runs (PoseNLP.kkt at 64 make_pose_workload poses cycled over the batch), dx, dc in U[1, 2], b standard normal; HIP events; microseconds;",
             "medians of the rounds, the legs alternating in one process.  A, A', A'', B: ONE launch per round; C: torch.linalg.solve on the dense K in chunks of %d." % CHUNK, ""]
    for r in recs:
        rr = r["rounds"]
        med = {k: float(np.median(v)) for k, v in rr.items()}
        lines.append("%s (B = %d, n = %d, m = %d; A: status %s, inertia (81, m, 0) in %d poses; B: iterations min / median / max %d / %d / %d)"
                     % ((r["shape"], r["B"], r["n"], r["m"], r["status"], r["inertia_wanted"]) + r["iterations"]))
        for k in rr:
            lines.append("  %-4s median %12.1f   range %12.1f .. %12.1f   per pose %8.3f   rounds: %s" % (k, med[k], min(rr[k]), max(rr[k]), med[k] / r["B"], us(rr[k])))
        below = max(rr["A"]) < min(rr["C"])
        lines.append("  A / C = %.4f (medians); every round of A below every round of C: %s" % (med["A"] / med["C"], "yes" if below else "NO — the condition is NOT met here"))
        lines.append("  A / B = %.4f (medians; reported, not required): the direct solve is %s than MINRES at these diagonals" % (med["A"] / med["B"], "faster" if med["A"] < med["B"] else "SLOWER"))
        lines.append("  max relative difference of the solutions (per pose, against its largest element): A against C %.2e, B against C %.2e; A'' bit for bit A: %s; A' inertia equal A's: %s"
                     % (r["a_c_diff"], r["b_c_diff"], r["a2_equal"], r["inertia_equal"]))
        lines.append("")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--emulation-only", action="store_true", help="the CPU emulation's table alone: no device")
    ap.add_argument("--out")
    ap.add_argument("--session", default=time.strftime("%Y-%m-%d %H:%M:%S"))
    a = ap.parse_args()
    head = emulation_section()

    def write(text):
        if a.out:                       # (after every shape: a run that is cut short leaves what it has)
            with open(a.out, "w") as f:
                f.write(text)
    if a.emulation_only:
        write(head + "\nTimings: UNMEASURED (this file was written without a device).\n")
        print(head)
        return
    recs = []
    for shape in [s for s in a.shapes.split(",") if s]:
        recs.append(probe(shape, a.rounds))
        print({k: v for k, v in recs[-1].items() if k != "rounds"}, flush=True)
        write(head + "\n" + report(recs, a.session))
    print(report(recs, a.session))


if __name__ == "__main__":
    main()
