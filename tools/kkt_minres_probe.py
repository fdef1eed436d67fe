#!/usr/bin/env python3
"""Microseconds per MINRES iteration on the KKT operator of a batch: the device-resident solve (KKTValues.solve, hipnlp_kkt_minres_device,
three launches per iteration) against the same recurrence written in torch around KKTValues.matvec, timed with HIP events.

    A = K.solve(b_top, b_bottom, rtol=0.0, maxiter=ITERS, check_every=0): the two launches of the start and 3 ITERS launches, no host
        synchronisation (rtol = 0: no trajectory freezes, every iteration does its work)
    B = the recurrence of hippopt_amd/csrc/knot_minres.h in torch on K.matvec: the scalars are [batch] device tensors, no .item(), no
        synchronisation; top and bottom halves are separate contiguous tensors because matvec takes them so (about 45 torch kernels and the
        operator's launch per iteration)

No preconditioner; value runs 0.05 standard_normal, dx, dc in U[1, 2], b standard normal (the conditioned inputs of the tests — the time
of an iteration does not depend on the values).  A round is one solve of ITERS iterations per leg, the legs alternating in one process;
its figure is elapsed / ITERS (the start included in both).  The solutions of A and B are compared once per shape."""
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


def settings_of(name, model):
    from hippopt_amd.kinodyn_settings import periodic_step_settings, stairs_settings
    if name.startswith("planar"):
        return periodic_step_settings(100, model), int(name.split("x")[1])
    return stairs_settings(200, model), 16


def torch_minres(torch, K, bt, bb, iters):
    """the recurrence of knot_minres.h for the identity preconditioner, `iters` iterations from a zero start; (z_top, z_bottom, phibar / beta1)"""
    col = lambda s: s[:, None]  # noqa: E731
    dot = lambda at, ab, ct, cb: torch.linalg.vecdot(at, ct) + torch.linalg.vecdot(ab, cb)  # noqa: E731
    r1t, r1b, r2t, r2b = bt, bb, bt, bb
    beta1 = beta = torch.sqrt(dot(bt, bb, bt, bb))
    oldb = dbar = epsln = torch.zeros_like(beta)
    phibar, cs, sn = beta1, -torch.ones_like(beta), torch.zeros_like(beta)
    wt, wb, w2t, w2b = torch.zeros_like(bt), torch.zeros_like(bb), torch.zeros_like(bt), torch.zeros_like(bb)
    zt, zb = torch.zeros_like(bt), torch.zeros_like(bb)
    for it in range(1, iters + 1):
        inv = col(1.0 / beta)
        vt, vb = r2t * inv, r2b * inv
        yt, yb = K.matvec(vt, vb)
        if it >= 2:
            c1 = col(beta / oldb)
            yt.addcmul_(r1t, c1, value=-1.0)
            yb.addcmul_(r1b, c1, value=-1.0)
        alfa = dot(vt, vb, yt, yb)
        c2 = col(alfa / beta)
        yt.addcmul_(r2t, c2, value=-1.0)
        yb.addcmul_(r2b, c2, value=-1.0)
        r1t, r1b, r2t, r2b = r2t, r2b, yt, yb
        oldb, beta = beta, torch.sqrt(dot(r2t, r2b, r2t, r2b))
        oldeps, delta, gbar = epsln, cs * dbar + sn * alfa, sn * dbar - cs * alfa
        epsln, dbar = sn * beta, -cs * beta
        gamma = torch.sqrt(gbar * gbar + beta * beta).clamp_min(sys.float_info.min)
        cs, sn = gbar / gamma, beta / gamma
        phi, phibar = cs * phibar, sn * phibar
        w1t, w1b, w2t, w2b = w2t, w2b, wt, wb
        ig = col(1.0 / gamma)
        wt = (vt - col(oldeps) * w1t - col(delta) * w2t) * ig
        wb = (vb - col(oldeps) * w1b - col(delta) * w2b) * ig
        zt.addcmul_(wt, col(phi))
        zb.addcmul_(wb, col(phi))
    return zt, zb, phibar / beta1


def probe(shape, rounds, iters):
    import torch
    from hippopt_amd.autograd import KKTValues, KinodynamicNLP
    from hippopt_amd.robot_model import synthetic_ergocub
    model = synthetic_ergocub()
    st, B = settings_of(shape, model)
    work = torch.cuda.Stream()        # (an explicit stream: on torch's default one the library would go to a side stream and back)
    with torch.cuda.stream(work):
        nlp = KinodynamicNLP(st, model, batch=B)
        eng = nlp.engine
        n, m, nnz, nnz_h = eng.n, eng.m, eng.nnz, eng.hess_nnz()
        gen = torch.Generator(device="cuda")
        gen.manual_seed(12)
        rn = lambda *s: torch.randn(s, dtype=torch.float64, device="cuda", generator=gen)  # noqa: E731
        un = lambda *s: 1.0 + torch.rand(s, dtype=torch.float64, device="cuda", generator=gen)  # noqa: E731
        K = KKTValues(nlp, 0.05 * rn(B, nnz_h), 0.05 * rn(B, nnz), un(B, n), un(B, m))
        bt, bb = rn(B, n), rn(B, m)
        workspace = eng.kkt_minres_reserve()

        def leg_a():
            return K.solve(bt, bb, rtol=0.0, maxiter=iters, check_every=0)

        def leg_b():
            return torch_minres(torch, K, bt, bb, iters)

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1000.0 / iters, out

        timed(leg_a)
        timed(leg_b)                  # warm-up: allocator, workspace, code objects
        res = {"A": [], "B": []}
        for _ in range(rounds):
            ta, za = timed(leg_a)
            tb, zb = timed(leg_b)
            res["A"].append(ta)
            res["B"].append(tb)
        diff = float(torch.maximum((za.top - zb[0]).abs().max(), (za.bottom - zb[1]).abs().max()))
        scale = float(torch.maximum(za.top.abs().max(), za.bottom.abs().max()))
        return {"shape": shape, "batch": B, "N": st.horizon_length, "n": n, "m": m, "nnz": nnz, "nnz_h": nnz_h, "iters": iters, "rounds": res, "workspace": workspace,
                "status": sorted(set(za.status.cpu().tolist())), "iterations": sorted(set(za.iterations.cpu().tolist())),
                "residual_a": float(za.residual.max()), "residual_b": float(zb[2].max()), "max_abs_diff": diff, "max_abs": scale}


def report(recs, session):
    lines = ["MINRES on the KKT operator, microseconds per iteration: the device-resident solve (A: K.solve(check_every=0), three launches per iteration) against the same",
             "recurrence in torch on K.matvec with the scalars as device tensors (B); identity preconditioner, conditioned synthetic value runs",
             "tools/kkt_minres_probe.py; box %s, session %s; one box, one session; a round is one solve, its figure elapsed / iterations (the start included)"
             % (socket.gethostname(), session), ""]
    fmt = lambda ts: " ".join("%.1f" % t for t in ts)  # noqa: E731
    for r in recs:
        rr = r["rounds"]
        med = {k: float(np.median(rr[k])) for k in rr}
        lines.append("%s (N = %d, B = %d, n = %d, m = %d, nnz = %d, nnz_h = %d; %d iterations per solve; workspace %.1f MB)"
                     % (r["shape"], r["N"], r["batch"], r["n"], r["m"], r["nnz"], r["nnz_h"], r["iters"], r["workspace"] / 1e6))
        lines.append("  A  (K.solve, check_every = 0)            median %8.1f   range %8.1f .. %8.1f   rounds: %s" % (med["A"], min(rr["A"]), max(rr["A"]), fmt(rr["A"])))
        lines.append("  B  (torch recurrence on K.matvec)        median %8.1f   range %8.1f .. %8.1f   rounds: %s" % (med["B"], min(rr["B"]), max(rr["B"]), fmt(rr["B"])))
        lines.append("  A / B = %.3f (medians); every A round below every B round: %s" % (med["A"] / med["B"], "yes" if max(rr["A"]) < min(rr["B"]) else "NO — the solve is NOT faster here"))
        lines.append("  A: status %s after %s iterations, residual up to %.3e; B: residual up to %.3e; max |z_A - z_B| = %.3e (max |z| = %.3e)"
                     % (r["status"], r["iterations"], r["residual_a"], r["residual_b"], r["max_abs_diff"], r["max_abs"]))
        lines.append("")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out")
    ap.add_argument("--session", default=time.strftime("%Y-%m-%d %H:%M:%S"))
    a = ap.parse_args()
    recs = []
    for shape in a.shapes.split(","):
        recs.append(probe(shape, a.rounds, a.iters))
        print(recs[-1]["shape"], {k: ["%.1f" % t for t in v] for k, v in recs[-1]["rounds"].items()}, flush=True)
    text = report(recs, a.session)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
