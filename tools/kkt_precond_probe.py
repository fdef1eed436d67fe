#!/usr/bin/env python3
"""The diagonal preconditioner of the KKT solve, built on the device (KKTValues.diagonal_preconditioner, hipnlp_kkt_diag_precond_device):
(a) microseconds per build against the same two vectors in torch, timed with HIP events; (b) what the diagonal does to K.solve on real
value runs.

(a)  A = K.diagonal_preconditioner(): the one launch.
     B = the same two vectors in torch: index_select of the Hessian diagonal out of the value run, + dx, abs, clamp_min, reciprocal; then
         (J o J) as ONE torch sparse CSR matrix of the whole batch (block diagonal, [batch m, batch n]) times minv_top, + dc, abs, clamp_min,
         reciprocal.  The CSR matrix — its pattern AND its squared values — is built once outside the timing: B does not pay for squaring
         the jac run or for bringing it into CSR order, which a caller with new values at every interior-point iteration would.
     Value runs 0.05 standard_normal, dx, dc in U[1, 2] (the time of a build does not depend on the values).  A round is REPS builds per
     leg, the legs alternating in one process; its figure is elapsed / REPS.  A and B are compared once per shape.
(b)  Iterations and status of K.solve(rtol=1e-8, maxiter=3000, check_every=50) with minv=None and with minv=K.diagonal_preconditioner(),
     on the KKT systems of synthetic workloads' iterates (nlp.kkt at make_workload(seed=8900), on the stairs with place_on_step_flanks;
     sigma = 0.8; lam, b standard normal; dx, dc in U[1, 2], one seed): the N = 4 systems of the tests (batch 3) and the shapes of (a).
     dx and dc are NOT those of an interior-point method (no Sigma = Z / X of a barrier iterate, no inertia correction): the records say
     what this diagonal does on these matrices, nothing about the cost of an interior-point step."""
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
SOLVE_SHAPES = ("planar_4x3", "stairs_4x3") + SHAPES
FLOOR = 1e-10
DEVICE = "cuda"


def settings_of(name, model):
    from hippopt_amd.kinodyn_settings import periodic_step_settings, stairs_settings
    kind, dims = name.split("_")
    horizon, batch = (int(t) for t in dims.split("x"))
    return (periodic_step_settings if kind == "planar" else stairs_settings)(horizon, model), batch


def hess_diagonal(torch, nlp, K):
    """diag H [batch, n] out of the value run (+0.0 where the pattern has no entry)"""
    hr, hc = (np.asarray(a) for a in nlp.engine.hess_sparsity())
    on = np.flatnonzero(hr == hc)
    hd = torch.zeros((nlp.batch, nlp.n), dtype=torch.float64, device=DEVICE)
    return hd.index_copy_(1, torch.tensor(hr[on], dtype=torch.int64, device=DEVICE), K.hess.index_select(1, torch.tensor(on, dtype=torch.int64, device=DEVICE)))


def torch_builder(torch, nlp, K):
    """B of (a): (a function () -> (top, bottom), how the sparse product is formed); everything that does not depend on dx / dc is
    prepared here, outside the timing"""
    eng = nlp.engine
    B, n, m = nlp.batch, nlp.n, nlp.m
    hr, hc = (np.asarray(a) for a in eng.hess_sparsity())
    ir, jc = (np.asarray(a) for a in eng.sparsity())
    on = np.flatnonzero(hr == hc)
    pos = torch.tensor(on, dtype=torch.int64, device=DEVICE)                   # the diagonal entries of the value run ...
    var = torch.tensor(hr[on], dtype=torch.int64, device=DEVICE)               # ... and their variables (the globals have none)
    order = np.lexsort((jc, ir))                                               # CSR order of one trajectory: by row, then ascending column
    crow = np.concatenate([[0], np.cumsum(np.bincount(ir, minlength=m))]).astype(np.int64)
    o = torch.tensor(order, dtype=torch.int64, device=DEVICE)
    step = torch.arange(B, dtype=torch.int64, device=DEVICE)
    col = (torch.tensor(jc[order], dtype=torch.int64, device=DEVICE)[None, :] + n * step[:, None]).reshape(-1)
    rows = torch.cat([(torch.tensor(crow[:-1], dtype=torch.int64, device=DEVICE)[None, :] + ir.size * step[:, None]).reshape(-1),
                      torch.tensor([B * ir.size], dtype=torch.int64, device=DEVICE)])
    jj = torch.sparse_csr_tensor(rows, col, (K.jac * K.jac).index_select(1, o).reshape(-1), size=(B * m, B * n))
    full = var.numel() == n
    vec = torch.ones(B * n, dtype=torch.float64, device=DEVICE)
    product, how = None, None
    for how, fn in (("torch.mv(csr, x)", lambda x: torch.mv(jj, x)), ("(csr @ x[:, None])[:, 0]", lambda x: (jj @ x[:, None])[:, 0])):
        try:
            fn(vec)
            product = fn
            break
        except (RuntimeError, NotImplementedError) as err:
            print("torch: %s is not available here (%s)" % (how, str(err).split("\n")[0]), flush=True)
    if product is None:           # no CSR product in this torch build: the same sum by index_add_ over the triplets
        how = "index_add_ over the triplets (this torch build has no sparse CSR product on the device)"
        vals, rix, cix = jj.values(), torch.tensor(np.tile(ir[order], B) + m * np.repeat(np.arange(B), ir.size), dtype=torch.int64, device=DEVICE), col
        product = lambda x: torch.zeros(B * m, dtype=torch.float64, device=DEVICE).index_add_(0, rix, vals * x.index_select(0, cix))  # noqa: E731

    def build():
        hd = K.hess.index_select(1, pos)
        if not full:
            hd = torch.zeros((B, n), dtype=torch.float64, device=DEVICE).index_copy_(1, var, hd)
        top = (hd + K.dx).abs_().clamp_min_(FLOOR).reciprocal_()
        s = product(top.reshape(-1)).reshape(B, m)
        return top, s.add_(K.dc).abs_().clamp_min_(FLOOR).reciprocal_()
    return build, how


def time_builds(shape, rounds, reps):
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
        gen = torch.Generator(device=DEVICE)
        gen.manual_seed(13)
        rn = lambda *s: torch.randn(s, dtype=torch.float64, device=DEVICE, generator=gen)  # noqa: E731
        un = lambda *s: 1.0 + torch.rand(s, dtype=torch.float64, device=DEVICE, generator=gen)  # noqa: E731
        K = KKTValues(nlp, 0.05 * rn(B, nnz_h), 0.05 * rn(B, nnz), un(B, n), un(B, m))
        leg_b, how = torch_builder(torch, nlp, K)

        def leg_a():
            return K.diagonal_preconditioner(FLOOR)

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                out = fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1000.0 / reps, out

        timed(leg_a)
        timed(leg_b)                  # warm-up: allocator, tables, code objects
        res = {"A": [], "B": []}
        for _ in range(rounds):
            ta, da = timed(leg_a)
            tb, db = timed(leg_b)
            res["A"].append(ta)
            res["B"].append(tb)
        rel = max(float(((da[i] - db[i]).abs() / db[i]).max()) for i in (0, 1))
        return {"shape": shape, "batch": B, "N": st.horizon_length, "n": n, "m": m, "nnz": nnz, "nnz_h": nnz_h, "reps": reps, "rounds": res, "max_rel_diff": rel, "product": how}


def solve_records(shape):
    import torch
    from hippopt_amd.autograd import KinodynamicNLP
    from hippopt_amd.robot_model import synthetic_ergocub
    from hippopt_amd.synthetic import make_workload, place_on_step_flanks
    model = synthetic_ergocub()
    st, B = settings_of(shape, model)
    x, p = make_workload(st, model, batch=B, seed=8900)
    if shape.startswith("stairs"):
        place_on_step_flanks(x[:1] if st.horizon_length == 4 else x, st, seed=3)      # (N = 4: trajectory 0 only, as the tests do)
    dev = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=DEVICE)  # noqa: E731
    work = torch.cuda.Stream()
    with torch.cuda.stream(work):
        nlp = KinodynamicNLP(st, model, batch=B)
        nlp.set_params(p)
        rng = np.random.RandomState(11)
        lam, dx, dc = rng.standard_normal((B, nlp.m)), rng.uniform(1.0, 2.0, (B, nlp.n)), rng.uniform(1.0, 2.0, (B, nlp.m))
        bt, bb = dev(rng.standard_normal((B, nlp.n))), dev(rng.standard_normal((B, nlp.m)))
        K = nlp.kkt(dev(x), 0.8, dev(lam), dev(dx), dev(dc))
        minv = K.diagonal_preconditioner(FLOOR)
        rec = {"shape": shape, "batch": B, "N": st.horizon_length, "n": nlp.n, "m": nlp.m, "max_hess": float(K.hess.abs().max()), "max_jac": float(K.jac.abs().max()),
               "negative": int(((hess_diagonal(torch, nlp, K) + K.dx) < 0).sum(1).max())}
        for key, mv in (("identity", None), ("built", minv)):
            t0 = time.time()
            z = K.solve(bt, bb, rtol=1e-8, maxiter=3000, minv=mv, check_every=50)
            torch.cuda.synchronize()
            status, its, res = z.status.cpu().numpy(), z.iterations.cpu().numpy(), z.residual.cpu().numpy()
            rec[key] = {"seconds": time.time() - t0, "status": {int(s): int((status == s).sum()) for s in np.unique(status)}, "iterations": (int(its.min()), int(np.median(its)), int(its.max())),
                        "residual": (float(res.min()), float(np.median(res)), float(res.max()))}
        return rec


def report(builds, solves, session):
    lines = ["The diagonal preconditioner of the KKT solve built on the device (tools/kkt_precond_probe.py); box %s, session %s; one box, one session" % (socket.gethostname(), session), "",
             "(a) microseconds per build: A = K.diagonal_preconditioner() (hipnlp_kkt_diag_precond_device, one launch) against B = the same two vectors in torch",
             "    (index_select of the diagonal, + dx, abs, clamp_min, reciprocal; (J o J) as one block-diagonal sparse CSR matrix of the batch times minv_top, + dc, abs,",
             "    clamp_min, reciprocal; the CSR matrix, squared values included, built once OUTSIDE the timing); a round is `reps` builds, its figure elapsed / reps", ""]
    fmt = lambda ts: " ".join("%.1f" % t for t in ts)  # noqa: E731
    for r in builds:
        rr = r["rounds"]
        med = {k: float(np.median(rr[k])) for k in rr}
        lines.append("%s (N = %d, B = %d, n = %d, m = %d, nnz = %d, nnz_h = %d; %d builds per round)" % (r["shape"], r["N"], r["batch"], r["n"], r["m"], r["nnz"], r["nnz_h"], r["reps"]))
        lines.append("  A  (one launch)                          median %8.1f   range %8.1f .. %8.1f   rounds: %s" % (med["A"], min(rr["A"]), max(rr["A"]), fmt(rr["A"])))
        lines.append("  B  (torch: gather, CSR product)          median %8.1f   range %8.1f .. %8.1f   rounds: %s" % (med["B"], min(rr["B"]), max(rr["B"]), fmt(rr["B"])))
        lines.append("  A / B = %.3f (medians); every A round below every B round: %s; max relative |A - B| = %.3e; B's product: %s"
                     % (med["A"] / med["B"], "yes" if max(rr["A"]) < min(rr["B"]) else "NO — the launch is NOT faster here", r["max_rel_diff"], r["product"]))
        lines.append("")
    lines += ["(b) K.solve(rtol=1e-8, maxiter=3000, check_every=50) on the KKT systems of synthetic workloads' iterates, without a preconditioner and with the built diagonal",
              "    (floor %g); sigma = 0.8, lam and b standard normal, dx and dc in U[1, 2] (NOT an interior-point method's), one seed.  Records, not requirements." % FLOOR,
              "    status: {status: trajectories}; iterations and residual: min / median / max over the batch", ""]
    for r in solves:
        lines.append("%s (N = %d, B = %d, n = %d, m = %d; max |H| %.2e, max |J| %.2e, up to %d negative diagonals of H + dx per trajectory)"
                     % (r["shape"], r["N"], r["batch"], r["n"], r["m"], r["max_hess"], r["max_jac"], r["negative"]))
        for key in ("identity", "built"):
            s = r[key]
            lines.append("  %-9s status %-16s iterations %4d / %4d / %4d   residual %.2e / %.2e / %.2e   (%.1f s)"
                         % ((key, str(s["status"])) + s["iterations"] + s["residual"] + (s["seconds"],)))
        lines.append("")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--solve-shapes", default=",".join(SOLVE_SHAPES))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out")
    ap.add_argument("--session", default=time.strftime("%Y-%m-%d %H:%M:%S"))
    a = ap.parse_args()
    builds, solves = [], []
    for shape in [s for s in a.shapes.split(",") if s]:
        builds.append(time_builds(shape, a.rounds, a.reps))
        print(builds[-1]["shape"], {k: ["%.1f" % t for t in v] for k, v in builds[-1]["rounds"].items()}, flush=True)
    for shape in [s for s in a.solve_shapes.split(",") if s]:
        solves.append(solve_records(shape))
        print(solves[-1], flush=True)
    text = report(builds, solves, a.session)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
