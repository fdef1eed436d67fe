"""The per-knot inertia-correcting ladder of the block factorisation (hippopt_amd/csrc/knot_ldl.h LADDER), run by the CPU emulation of
hipnlp_kkt_block_ladder_kernel (tests/kkt_ladder_emu), on the real N = 4 value runs of tests/test_kkt_block_hostemu.py::real_runs (stairs and
periodic; dx, dc in U[1, 2]):

  the ladder against a hand loop over ONE factorisation at an explicit delta, bit for bit; try 0 against block_factor;
  against numpy: eigvalsh(block + delta_k I) all positive, and not all positive at the previous try's delta;
  the dense convexified K' has eigvalsh sign counts (n, m, 0);
  after a successful ladder every pivot is 1x1, o = 0, e = 1 / d, and block_apply is the inverse of the dense H_k + dx_k + delta_k I;
  a zero column, a NaN knot, an exhausted ladder, max_tries = 0, N = 2;
  MINRES on the convexified system with the ladder's preconditioner: status 0 implies a true residual within 100 rtol.

CHOSEN for these tests: delta_init = 1e-4, kappa = 8 (convexify's defaults, IPOPT's first_hessian_perturbation and perturb_inc_fact), floor
1e-10, max_tries 16.  SEEN with them: stairs N = 4 tries [11, 14, 12, 13], delta [1.07e5, 5.50e7, 8.59e5, 6.87e6]; periodic N = 4 tries
[8, 8, 7, 6], delta [209.7, 209.7, 26.2, 3.28]; every knot status 0.  Of the 54 + 33 (knot, try) pairs none is undecidable for the
reference (smallest |eigenvalue| below 189 2^-53 max |eigenvalue|); the cap is one in ten.  (delta_init = 1e-2, kappa = 4 exhausts stairs
knot 1 at try 16; delta_init = 1e-3, kappa = 2 exhausts all four.)  The stairs' delta is large because H_k has eigenvalues down to
about -1e7 there: the ladder makes the whole block positive definite, which IPOPT's criterion does not ask for.  CPU only."""
import numpy as np
import pytest

import kkt_check
import pose_ldl_check as plc
from kkt_check import bits
from kkt_emu_lib import NXK
from test_kkt_block_hostemu import dense_block, real_runs, split
from test_kkt_minres_hostemu import inputs
from test_lagrangian_grad_hostemu import MAKERS

U = 2.0 ** -53
FLOOR, DELTA_INIT, KAPPA, MAX_TRIES = 1e-10, 1e-4, 8.0, 16
WANTED = [NXK, 0, 0]
REAL = ["stairs", "periodic"]
RECORD = ("factor", "words", "e", "o", "inertia")
_EMU, _LADDER = {}, {}


def emu_of(model, name, horizon):
    from kkt_ladder_emu_lib import KktLadderEmu
    if (name, horizon) not in _EMU:
        _EMU[name, horizon] = KktLadderEmu(MAKERS[name](horizon, model), model)
    return _EMU[name, horizon]


def runs(model, name, horizon=4):
    """(this emulation, patterns, inputs) of real_runs: its patterns and inputs, computed once and left unchanged"""
    _, pat, d = real_runs(model, name, horizon)
    return emu_of(model, name, horizon), pat, d


def ladder_of(model, name, horizon=4):
    if (name, horizon) not in _LADDER:
        emu, pat, d = runs(model, name, horizon)
        _LADDER[name, horizon] = emu.block_ladder(d["hess"], d["dx"], FLOOR, DELTA_INIT, KAPPA, MAX_TRIES)
    return _LADDER[name, horizon]


def same_record(a, b, k, kb=None):
    """knot k of a Ladder / Block against knot kb of another, or against a Try"""
    for f in RECORD:
        x, y = getattr(a, f)[k], getattr(b, f) if kb is None else getattr(b, f)[kb]
        if not np.array_equal(bits(x) if x.dtype == np.float64 else x, bits(y) if y.dtype == np.float64 else y):
            return False
    return True


def hand_ladder(emu, hess, dx, k, delta_init, kappa, max_tries):
    """(the last Try, status, delta, tries, [(delta, inertia) of every try]) of knot k by a python loop over the single-delta factorisation"""
    from kkt_ladder_emu_lib import next_delta
    delta, t, seen = 0.0, 0, []
    while True:
        tr = emu.factor_at(k, hess, dx, FLOOR, None if t == 0 else delta)
        wanted = tr.inertia.tolist() == WANTED
        seen.append((delta, tr.inertia.tolist()))
        if tr.status == 2 or wanted or t >= max_tries:
            break
        t += 1
        delta = next_delta(t, delta, delta_init, kappa)
    status = tr.status if tr.status != 0 else (3 if max_tries > 0 and not wanted else 0)
    return tr, status, delta, t, seen


# ---- 1. the ladder against a hand loop ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", REAL)
def test_the_ladder_equals_a_hand_loop_over_single_factorisations(model, name):
    emu, pat, d = runs(model, name)
    lad = ladder_of(model, name)
    blk = emu.block_factor(d["hess"], d["dx"], FLOOR)
    assert lad.det_not_negative == 0 and lad.not_positive_definite == 0
    for k in range(emu.N):
        tr, status, delta, t, seen = hand_ladder(emu, d["hess"], d["dx"], k, DELTA_INIT, KAPPA, MAX_TRIES)
        print("%s knot %d: tries %d, delta %.6e, status %d; per try %s" % (name, k, t, delta, status, [(("%.3e" % dl), i) for dl, i in seen]))
        assert same_record(lad, tr, k), (name, k)
        assert (int(lad.status[k]), int(lad.tries[k])) == (status, t) and bits(lad.delta[k:k + 1])[0] == bits([delta])[0], (name, k)
        assert [i == WANTED for _, i in seen].index(True) == t                       # the FIRST try with the wanted inertia
        assert same_record(blk, emu.factor_at(k, d["hess"], d["dx"], FLOOR, None), k)   # try 0 is block_factor
    assert np.all(lad.status == 0) and np.all(lad.tries >= 1) and np.all(lad.tries <= MAX_TRIES)


# ---- 2. against numpy --------------------------------------------------------------------------------------------------------------------------------
def undecidable(ev):
    return np.abs(ev).min() < NXK * U * np.abs(ev).max()


def test_the_reference_alone_decides_at_least_nine_pairs_in_ten(model):
    from kkt_ladder_emu_lib import next_delta
    pairs = skipped = 0
    for name in REAL:
        emu, pat, d = runs(model, name)
        for k in range(emu.N):
            A, delta = dense_block(pat, d["hess"], d["dx"], k), 0.0
            for t in range(MAX_TRIES + 1):
                delta = delta if t == 0 else next_delta(t, delta, DELTA_INIT, KAPPA)
                ev = np.linalg.eigvalsh(A + delta * np.eye(NXK))
                pairs += 1
                skipped += bool(undecidable(ev))
    print("undecidable (knot, try) pairs: %d of %d" % (skipped, pairs))
    assert 10 * skipped <= pairs


@pytest.mark.parametrize("name", REAL)
def test_delta_makes_the_block_positive_definite_and_the_try_before_did_not(model, name):
    from kkt_ladder_emu_lib import next_delta
    emu, pat, d = runs(model, name)
    lad = ladder_of(model, name)
    pairs = skipped = 0
    for k in range(emu.N):
        assert lad.status[k] == 0 and lad.inertia[k].tolist() == WANTED
        A = dense_block(pat, d["hess"], d["dx"], k)
        deltas = [0.0]
        for t in range(1, int(lad.tries[k]) + 1):
            deltas.append(next_delta(t, deltas[-1], DELTA_INIT, KAPPA))
        assert bits(np.array([deltas[-1]]))[0] == bits(lad.delta[k:k + 1])[0]
        ev = np.linalg.eigvalsh(A + deltas[-1] * np.eye(NXK))
        pairs += 1
        print("%s knot %d: tries %d, delta %.4e, eigvalsh(block + delta I) in [%.3e, %.3e]" % (name, k, lad.tries[k], deltas[-1], ev.min(), ev.max()))
        if undecidable(ev):
            skipped += 1
        else:
            assert np.all(ev > 0.0), (name, k, ev.min())
        if lad.tries[k] >= 1:
            before = np.linalg.eigvalsh(A + deltas[-2] * np.eye(NXK))
            pairs += 1
            if undecidable(before):
                skipped += 1
            else:
                assert before.min() <= 0.0, (name, k, before.min())
    assert 10 * skipped <= pairs, (skipped, pairs)


# ---- 3. quasi-definiteness ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", REAL)
def test_the_convexified_system_has_the_inertia_n_m_0(model, name):
    emu, pat, d = runs(model, name)
    lad = ladder_of(model, name)
    assert emu.n + emu.m < 2000
    K = kkt_check.dense(emu.n, emu.m, *pat[:2], d["hess"], *pat[2:], d["jac"], emu.convexified_dx(d["dx"], lad.delta), d["dc"])
    ev = np.linalg.eigvalsh(K)
    counts = (int((ev > 0).sum()), int((ev < 0).sum()), int((ev == 0).sum()))
    ev0 = np.linalg.eigvalsh(kkt_check.dense(emu.n, emu.m, *pat[:2], d["hess"], *pat[2:], d["jac"], d["dx"], d["dc"]))
    print("%s: convexified K' signs %s, smallest |eigenvalue| %.3e; the original K %s" % (name, counts, np.abs(ev).min(), ((ev0 > 0).sum(), (ev0 < 0).sum(), (ev0 == 0).sum())))
    assert counts == (emu.n, emu.m, 0)
    assert (int((ev0 > 0).sum()), int((ev0 < 0).sum())) != (emu.n, emu.m)             # (the original K is not: the ladder had something to do)


# ---- 4. the stored factor is the exact inverse -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", REAL)
def test_after_the_ladder_every_pivot_is_one_by_one_and_apply_inverts_the_dense_block(model, name):
    from kkt_block_emu_lib import PL_ONE, word_kind
    emu, pat, d = runs(model, name)
    lad = ladder_of(model, name)
    dxp = emu.convexified_dx(d["dx"], lad.delta)
    diag = emu.diagonal_preconditioner(d["hess"], d["jac"], dxp, d["dc"], FLOOR)
    r = np.random.RandomState(17).standard_normal(emu.n)
    a = emu.block_apply(lad, (diag.top, diag.bottom), r, d["bb"])
    assert np.all(a.top_writes == 1) and np.all(a.bottom_writes == 1)
    for k in range(emu.N):
        assert np.all(word_kind(lad.words[k]) == PL_ONE) and np.all(lad.o[k] == 0.0), (name, k)
        L, D, perm, kind = split(lad, k)
        dd = np.diag(D)
        assert np.all(dd > FLOOR) and np.array_equal(bits(lad.e[k]), bits(1.0 / dd)), (name, k)
        A = dense_block(pat, d["hess"], d["dx"], k) + lad.delta[k] * np.eye(NXK)
        b, z = r[NXK * k:NXK * (k + 1)], a.top[NXK * k:NXK * (k + 1)]
        bound, ref = plc.eta_bound(A, b)
        got = plc.eta(A, z, b)
        print("%s knot %d: eta %.3e, numpy's %.3e, bound %.3e" % (name, k, got, ref, bound))
        assert bound == max(16.0 * ref, NXK * U) and got <= bound, (name, k, got, bound)


# ---- 5. edges ------------------------------------------------------------------------------------------------------------------------------------------------
def test_an_exactly_zero_column_becomes_positive_at_a_later_try(model):
    """tests/test_kkt_block_hostemu.py's construction: variable 17 of knot 1 of the synthetic stairs N = 3 runs has no entry and dx = 0"""
    emu = emu_of(model, "stairs", 3)
    hr, hc = (np.asarray(a) for a in emu.hess_sparsity())
    d = inputs(emu, 903)
    c = NXK * 1 + 17
    hess, dx = d["hess"].copy(), d["dx"].copy()
    hess[(hr == c) | (hc == c)] = 0.0
    dx[c] = 0.0
    once = emu.block_ladder(hess, dx, FLOOR, DELTA_INIT, KAPPA, 0)
    assert once.status.tolist() == [0, 0, 0] and once.inertia[:, 2].tolist() == [0, 1, 0] and once.tries.tolist() == [0, 0, 0]
    lad = emu.block_ladder(hess, dx, FLOOR, DELTA_INIT, KAPPA, MAX_TRIES)
    assert lad.status.tolist() == [0, 0, 0] and lad.tries.tolist() == [0, 1, 0] and lad.delta.tolist() == [0.0, DELTA_INIT, 0.0]
    assert np.all(lad.inertia == WANTED)
    from kkt_block_emu_lib import word_perm
    at = int(np.flatnonzero(word_perm(lad.words[1]) == 17)[0])
    assert lad.e[1][at] == 1.0 / DELTA_INIT                                      # the pivot of the column that was zero is delta itself


def test_a_nan_knot_has_status_2_and_the_others_keep_their_bits(model):
    emu, pat, d = runs(model, "stairs")
    clean = ladder_of(model, "stairs")
    nnz_knot = emu.block_pattern()[1].size
    hess = d["hess"].copy()
    hess[2 * nnz_knot + 5] = np.nan
    lad = emu.block_ladder(hess, d["dx"], FLOOR, DELTA_INIT, KAPPA, MAX_TRIES)
    assert lad.status.tolist() == [0, 0, 2, 0] and lad.tries[2] == 0 and lad.delta[2] == 0.0 and lad.inertia[2].tolist() == [0, 0, 0]
    assert np.all(np.isnan(lad.factor[2])) and np.all(np.isnan(lad.e[2])) and np.all(np.isnan(lad.o[2]))
    assert np.array_equal(lad.words[2], (np.arange(NXK) + 1) | (np.arange(NXK) << 16))
    for k in (0, 1, 3):
        assert same_record(lad, clean, k, k) and lad.tries[k] == clean.tries[k] and lad.delta[k] == clean.delta[k] and lad.status[k] == 0, k


@pytest.mark.parametrize("name", REAL)
def test_one_try_of_a_tiny_delta_is_exhausted_with_that_trys_inertia(model, name):
    emu, pat, d = runs(model, name)
    lad = emu.block_ladder(d["hess"], d["dx"], FLOOR, 1e-300, KAPPA, 1)
    assert lad.status.tolist() == [3] * emu.N and lad.tries.tolist() == [1] * emu.N and lad.delta.tolist() == [1e-300] * emu.N
    for k in range(emu.N):
        tr = emu.factor_at(k, d["hess"], d["dx"], FLOOR, 1e-300)
        assert same_record(lad, tr, k) and tr.inertia.sum() == NXK and tr.inertia[1] > 0, (name, k)


@pytest.mark.parametrize("name", REAL)
def test_no_tries_is_block_factor(model, name):
    emu, pat, d = runs(model, name)
    for dx in (d["dx"], None):
        blk = emu.block_factor(d["hess"], dx, FLOOR)
        lad = emu.block_ladder(d["hess"], dx, FLOOR, float("nan"), float("nan"), 0)      # (delta_init and kappa are not read)
        for k in range(emu.N):
            assert same_record(lad, blk, k, k), (name, k)
        assert np.array_equal(lad.status, blk.status) and np.all(lad.status == 0) and np.all(lad.tries == 0) and np.all(bits(lad.delta) == 0)
        assert lad.inertia[:, 1].sum() > 0                                       # status 0 whatever the inertia


@pytest.mark.parametrize("name", REAL)
def test_two_knots_first_and_last_only(model, name):
    emu, pat, d = runs(model, name, 2)
    lad = ladder_of(model, name, 2)
    print("%s N=2: tries %s delta %s" % (name, lad.tries.tolist(), lad.delta.tolist()))
    assert lad.status.tolist() == [0, 0] and np.all(lad.inertia == WANTED)
    for k in range(2):
        tr, status, delta, t, seen = hand_ladder(emu, d["hess"], d["dx"], k, DELTA_INIT, KAPPA, MAX_TRIES)
        assert same_record(lad, tr, k) and (status, t) == (0, int(lad.tries[k])) and delta == lad.delta[k]
        assert np.all(np.linalg.eigvalsh(dense_block(pat, d["hess"], d["dx"], k) + delta * np.eye(NXK)) > 0.0)
    K = kkt_check.dense(emu.n, emu.m, *pat[:2], d["hess"], *pat[2:], d["jac"], emu.convexified_dx(d["dx"], lad.delta), d["dc"])
    ev = np.linalg.eigvalsh(K)
    assert (int((ev > 0).sum()), int((ev < 0).sum())) == (emu.n, emu.m)


# ---- 6. the solve on the convexified system ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", REAL)
def test_a_converged_solve_on_the_convexified_system_has_a_true_residual_within_100_rtol(model, name):
    """rtol 1e-8, as tests/test_kkt_block_hostemu.py, which allows a true residual of 1e-6 = 100 rtol.  No iteration count is asserted:
    profiles/r17_kkt_ladder.txt has them (tools/kkt_ladder_probe.py --emulation), beside the un-laddered block preconditioner's."""
    emu, pat, d = runs(model, name)
    lad = ladder_of(model, name)
    dxp = emu.convexified_dx(d["dx"], lad.delta)
    diag = emu.diagonal_preconditioner(d["hess"], d["jac"], dxp, d["dc"], FLOOR)
    rtol = 1e-8
    s = emu.block_solve(d["hess"], d["jac"], d["bt"], d["bb"], lad, (diag.top, diag.bottom), dx=dxp, dc=d["dc"], rtol=rtol, maxiter=3000)
    K = kkt_check.dense(emu.n, emu.m, *pat[:2], d["hess"], *pat[2:], d["jac"], dxp, d["dc"])
    b = np.concatenate([d["bt"], d["bb"]])
    true = float(np.linalg.norm(K @ np.concatenate([s.top, s.bottom]) - b) / np.linalg.norm(b))
    print("%s N=4 convexified: status %d after %d iterations, residual %.3e, true %.3e" % (name, s.status, s.iterations, s.residual, true))
    assert s.status in (0, 1)
    if s.status == 0:
        assert true <= 100.0 * rtol
    assert np.all(s.top_writes >= 1) and np.all(s.bottom_writes >= 1)
