#!/usr/bin/env python3
"""The KKT chain of the pose finder on the REAL value runs of a batch of poses (PoseNLP.kkt at make_pose_workload iterates; sigma in
U[0.5, 1.5], lam and b standard normal, dx and dc in U[1, 2] — NOT an interior-point method's), timed with HIP events (torch.cuda.Event)
on one explicit stream, `--rounds` rounds per leg, the legs alternating in one process; medians of the rounds, every round printed.

    A50    K.solve(rtol=0, maxiter=50, minv="diagonal"): 50 iterations forced.                       ONE launch per round.
    Aconv  K.solve(rtol=1e-8, maxiter=1000, minv="diagonal"): every pose to its own convergence.     ONE launch per round.
    B1     the same recurrence in torch on PoseKKTValues.matvec, the scalars as [batch] tensors, the diagonal given (built outside the
           timing): B1-50 runs 50 iterations, B1-conv as many as the slowest pose of Aconv took (a converged pose is frozen by a mask;
           nothing waits for the host).  Per iteration ONE operator launch and 67 torch kernels (counted from torch_minres below, whose
           lines carry their counts: elementwise kernels over the two halves of the vectors, four reductions, the [batch] scalars), so a
           round is 68 x iterations launches.
    B2     torch.linalg.solve on the dense [batch, n + m, n + m] K (assembly outside the timing): one call per round, rocSOLVER's launches
           inside it are not counted.  A direct solve: it is exact where MINRES stops at rtol.
    op     K.matvec(v, w) alone, diag  K.diagonal_preconditioner() alone: `--reps` launches per round, the figure is elapsed / reps.

    python tools/pose_kkt_probe.py --out profiles/r14_pose_kkt.txt"""
import argparse
import os
import socket
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for q in (ROOT, os.path.join(ROOT, "tests")):
    if q not in sys.path:
        sys.path.insert(0, q)

SHAPES = ("planar_4096", "planar_16384", "steps_4096", "steps_16384")
DEVICE = "cuda"
B1_KERNELS_PER_ITERATION = 67


def torch_minres(torch, K, b, minv, iters, rtol):
    """the recurrence of knot_minres.h on pairs (top, bottom) of [batch, .] tensors; returns (z pair, iterations [batch], phibar / beta1)"""
    dot = lambda p, q: (p[0] * q[0]).sum(1) + (p[1] * q[1]).sum(1)  # noqa: E731
    r1, r2 = b, b
    y = [minv[0] * b[0], minv[1] * b[1]]
    beta1 = beta = torch.sqrt(dot(r2, y))
    oldb = dbar = epsln = torch.zeros_like(beta)
    phibar, cs, sn = beta1, -torch.ones_like(beta), torch.zeros_like(beta)
    w = w2 = z = [torch.zeros_like(b[0]), torch.zeros_like(b[1])]
    done = beta1 == 0
    its = torch.zeros_like(beta, dtype=torch.int32)
    tiny = torch.full_like(beta, 2.2250738585072014e-308)
    for it in range(1, iters + 1):
        c = (1.0 / beta)[:, None]
        v = [y[0] * c, y[1] * c]                                                                    # 3
        y = list(K.matvec(v[0], v[1]))                                                              # the operator launch
        if it >= 2:
            c1 = (beta / oldb)[:, None]
            y = [y[0] - c1 * r1[0], y[1] - c1 * r1[1]]                                              # 5 (addcmul would make it 3)
        alfa = dot(v, y)                                                                            # 5
        c2 = (alfa / beta)[:, None]
        y = [y[0] - c2 * r2[0], y[1] - c2 * r2[1]]                                                  # 5
        r1, r2 = r2, y
        y = [minv[0] * r2[0], minv[1] * r2[1]]                                                      # 2
        oldb = beta
        beta = torch.sqrt(dot(r2, y))                                                               # 6
        oldeps, delta, gbar = epsln, cs * dbar + sn * alfa, sn * dbar - cs * alfa                   # 6
        epsln, dbar = sn * beta, -cs * beta                                                         # 3
        gamma = torch.maximum(torch.sqrt(gbar * gbar + beta * beta), tiny)                          # 5
        cs, sn = gbar / gamma, beta / gamma                                                         # 2
        phi, phibar = cs * phibar, sn * phibar                                                      # 2
        w1, w2 = w2, w
        g, oe, de, ph, keep = (1.0 / gamma)[:, None], oldeps[:, None], delta[:, None], phi[:, None], done[:, None]
        w = [(v[0] - oe * w1[0] - de * w2[0]) * g, (v[1] - oe * w1[1] - de * w2[1]) * g]            # 11
        z = [torch.where(keep, z[0], z[0] + ph * w[0]), torch.where(keep, z[1], z[1] + ph * w[1])]  # 6
        its = its + (~done).to(torch.int32)                                                         # 3
        done = done | (phibar <= rtol * beta1)                                                      # 3
    return z, its, phibar / beta1


def dense_k(torch, nlp, K):
    """[batch, n + m, n + m] from the two value runs and the diagonals"""
    n, m, B = nlp.n, nlp.m, nlp.batch
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.int64, device=DEVICE)  # noqa: E731
    hr, hc = (t(a) for a in nlp.engine.hess_sparsity())
    ir, jc = (t(a) for a in nlp.engine.sparsity())
    D = torch.zeros((B, n + m, n + m), dtype=torch.float64, device=DEVICE)
    D[:, hr, hc] = K.hess
    D[:, hc, hr] = K.hess
    D[:, n + ir, jc] = K.jac
    D[:, jc, n + ir] = K.jac
    i, j = torch.arange(n, device=DEVICE), n + torch.arange(m, device=DEVICE)
    D[:, i, i] += K.dx
    D[:, j, j] = -K.dc
    return D


def probe(shape, rounds, reps, with_dense):
    import torch
    from hippopt_amd.autograd import PoseNLP
    from hippopt_amd.pose_settings import make_pose_workload
    from hippopt_amd.robot_model import synthetic_ergocub
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
        minv = K.diagonal_preconditioner()
        conv = K.solve(bt, bb, rtol=1e-8, maxiter=1000, minv="diagonal")
        torch.cuda.synchronize()
        its, status = conv.iterations.cpu().numpy(), conv.status.cpu().numpy()
        iters_conv = int(its.max())
        rec = {"shape": shape, "B": B, "n": n, "m": m, "nnz": nlp.engine.nnz, "nnz_h": nlp.hess_nnz, "iterations": (int(its.min()), int(np.median(its)), iters_conv),
               "status": {int(s): int((status == s).sum()) for s in np.unique(status)}, "reps": reps, "max_hess": float(K.hess.abs().max())}
        legs = {"A50": (1, lambda: K.solve(bt, bb, rtol=0.0, maxiter=50, minv="diagonal")), "Aconv": (1, lambda: K.solve(bt, bb, rtol=1e-8, maxiter=1000, minv="diagonal")),
                "B1-50": (1, lambda: torch_minres(torch, K, (bt, bb), minv, 50, 0.0)), "B1-conv": (1, lambda: torch_minres(torch, K, (bt, bb), minv, iters_conv, 1e-8)),
                "op": (reps, lambda: K.matvec(bt, bb)), "diag": (reps, lambda: K.diagonal_preconditioner())}
        if with_dense:
            D = dense_k(torch, nlp, K)
            rhs = torch.cat([bt, bb], 1)[:, :, None]
            # the largest chunk of the batch this torch build's batched LU takes (hipBLAS's getrfBatched has refused 4 096 systems of 170 with
            # HIPBLAS_STATUS_ALLOC_FAILED): a round of B2 is then B / chunk calls
            for chunk in (B, 1024, 256, 64):
                try:
                    torch.linalg.solve(D[:chunk], rhs[:chunk])
                    torch.cuda.synchronize()
                except RuntimeError as err:
                    rec.setdefault("b2_refused", []).append("%d: %s" % (chunk, str(err).split("\n")[0][:160]))
                    continue
                rec["b2_chunk"] = chunk
                legs["B2"] = (1, lambda: torch.cat([torch.linalg.solve(D[i:i + chunk], rhs[i:i + chunk]) for i in range(0, B, chunk)]))
                break

        def timed(count, fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(count):
                out = fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1000.0 / count, out
        outs = {k: timed(c, fn)[1] for k, (c, fn) in legs.items()}        # warm-up: allocator, code objects, rocSOLVER's handle
        rec["rounds"] = {k: [] for k in legs}
        for _ in range(rounds):
            for k, (c, fn) in legs.items():
                rec["rounds"][k].append(timed(c, fn)[0])
        # that the legs compute the same thing
        zt = torch.cat([conv.top, conv.bottom], 1)
        zb = torch.cat(outs["B1-conv"][0], 1)
        scale = zt.abs().amax(1)
        rec["b1_diff"] = float(((zt - zb).abs().amax(1) / scale).max())
        rec["b1_its_equal"] = float((outs["B1-conv"][1].cpu().numpy() == its).mean())
        if "B2" in legs:
            rec["b2_diff"] = float(((zt - outs["B2"][:, :, 0]).abs().amax(1) / scale).max())
        return rec


def report(recs, session):
    us = lambda ts: " ".join("%.1f" % t for t in ts)  # noqa: E731
    lines = ["The KKT chain of the pose finder, one workgroup per pose (tools/pose_kkt_probe.py); box %s, session %s; one box, one session" % (socket.gethostname(), session),
             "Real value runs (PoseNLP.kkt at 64 make_pose_workload poses cycled over the batch), dx, dc in U[1, 2], b standard normal; HIP events; microseconds;",
             "medians of the rounds, the legs alternating in one process.  Launches per round: A50, Aconv ONE; B1 68 x iterations (one operator launch and %d torch"
             % B1_KERNELS_PER_ITERATION,
             "kernels per iteration); B2 torch.linalg.solve on the dense K in the chunks of its B2 line (assembled outside the timing; the launches inside a call are not counted); op and diag",
             "`reps` launches, figure per launch.", ""]
    for r in recs:
        rr = r["rounds"]
        med = {k: float(np.median(v)) for k, v in rr.items()}
        lines.append("%s (B = %d, n = %d, m = %d, nnz = %d, nnz_h = %d; max |H| %.1e; Aconv: status %s, iterations min / median / max %d / %d / %d)"
                     % ((r["shape"], r["B"], r["n"], r["m"], r["nnz"], r["nnz_h"], r["max_hess"], r["status"]) + r["iterations"]))
        for k in rr:
            lines.append("  %-8s median %12.1f   range %12.1f .. %12.1f   rounds: %s" % (k, med[k], min(rr[k]), max(rr[k]), us(rr[k])))
        for a, b in (("A50", "B1-50"), ("Aconv", "B1-conv"), ("A50", "B2"), ("Aconv", "B2")):
            if b in rr:
                faster = max(rr[a]) < min(rr[b])
                lines.append("  %-5s / %-7s = %.4f (medians); every A round below every B round: %s" % (a, b, med[a] / med[b], "yes" if faster else "NO — the one launch is NOT faster here"))
        lines.append("  per iteration: A50 %.2f us, B1-50 %.1f us; op alone %.1f us, diag alone %.1f us per launch (%d per round)"
                     % (med["A50"] / 50.0, med["B1-50"] / 50.0, med["op"], med["diag"], r["reps"]))
        lines.append("  max relative difference of the solutions (per pose, against its largest element): Aconv against B1-conv %.2e (same iteration count in %.1f %% of the poses)%s"
                     % (r["b1_diff"], 100.0 * r["b1_its_equal"], ("; against B2 %.2e" % r["b2_diff"]) if "b2_diff" in r else ""))
        if "b2_chunk" in r or "b2_refused" in r:
            lines.append("  B2: %s%s" % ("torch.linalg.solve on chunks of %d systems, %d calls per round" % (r["b2_chunk"], r["B"] // r["b2_chunk"]) if "b2_chunk" in r else "NOT MEASURED",
                                      "".join("; refused at " + t for t in r.get("b2_refused", []))))
        lines.append("")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-dense", action="store_true", help="leave B2 out")
    ap.add_argument("--out")
    ap.add_argument("--session", default=time.strftime("%Y-%m-%d %H:%M:%S"))
    a = ap.parse_args()
    recs = []
    for shape in [s for s in a.shapes.split(",") if s]:
        recs.append(probe(shape, a.rounds, a.reps, not a.no_dense))
        print({k: v for k, v in recs[-1].items() if k != "rounds"}, flush=True)
        text = report(recs, a.session)
        if a.out:                       # (after every shape: a run that is cut short leaves what it has)
            with open(a.out, "w") as f:
                f.write(text)
    print(report(recs, a.session))


if __name__ == "__main__":
    main()
