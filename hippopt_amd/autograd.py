"""torch autograd for the kinodynamic NLP of a batch of trajectories on one device.

    nlp = KinodynamicNLP(settings, model, batch=B)        # one engine handle (hipnlp_create) on cuda:`device`
    nlp.set_params(p)                                      # [B, np]
    f, g = nlp(x)                                          # x: [B, n] float64 cuda tensor -> f [B], g [B, m]
    loss = a * f.sum() + (w * g).sum()
    loss.backward()                                        # x.grad = a grad f + J^T w, ONE launch (hipnlp_eval_lagrangian_grad_device)

    hv = nlp.hessian_vector_product(x, sigma, lam, v)      # H(x, sigma, lam) v, ONE launch (hipnlp_eval_hess_vec_device), H never written
    H = nlp.hessian(x, sigma, lam)                         # the value run [B, nnz_h] (hipnlp_eval_hess_device), for many products at one x
    hv = H.matvec(v)                                       # hipnlp_hess_times_device: bit for bit the fused product

    J = nlp.jacobian(x)                                    # grad f [B, n] and the value run of jac g [B, nnz] (ONE hipnlp_eval_device launch)
    jv = J.matvec(v)                                       # J v [B, m]                 (hipnlp_jac_times_device)
    dot, jv = J.jvp(v)                                     # grad f . v [B] and J v in one launch
    gx = J.rmatvec(sigma, lam)                             # sigma grad f + J^T lam     (hipnlp_jac_transpose_times_device)
    dot, jv = nlp.jacobian_vector_product(x, v)            # the two launches above (evaluate, multiply) in one call

    K = nlp.kkt(x, sigma, lam, dx, dc)                     # the KKT operator [[H + diag dx, J^T], [J, -diag dc]] at one x: the two value runs
    top, bottom = K.matvec(v, w)                           # (H + diag dx) v + J^T w [B, n] and J v - dc w [B, m], ONE launch (hipnlp_kkt_times_device)
    K2 = K.with_diagonals(dx2, dc2)                        # other diagonals on the same value runs: no launch
    z = K.solve(b_top, b_bottom, rtol=1e-8, maxiter=200)   # K [z.top; z.bottom] = b by MINRES on the device (hipnlp_kkt_minres_device); z.status
    z = K.solve(b_top, b_bottom, minv=K.diagonal_preconditioner())   # ... with the diagonal M^-1 built in ONE launch (hipnlp_kkt_diag_precond_device)
    M = K.block_preconditioner()                           # per-knot L |D| L^T of H + diag dx (hipnlp_kkt_block_factor_device) + that diagonal; M.inertia
    z = K.solve(b_top, b_bottom, minv=M)                   # ... MINRES with the block top (hipnlp_kkt_minres_block_device)
    P = K.convexify()                                      # per-knot inertia-correcting ladder (hipnlp_kkt_block_ladder_device): P.delta, P.tries, P.quasi_definite
    z = P.values.solve(b_top, b_bottom, minv=P)            # ... MINRES on the convexified operator P.values with the exact inverse of its top blocks
    Cp = K.condensed_preconditioner()                      # per-knot L |D| L^T of B_k = H_k + dx_k + J_k^T diag(1/dc) J_k (hipnlp_kkt_condensed_factor_device); needs dc
    z = K.solve(b_top, b_bottom, minv=Cp)                  # ... MINRES with the condensed block top and 1/dc at the bottom; Cp.inertia: see its docstring

The forward pass is hipnlp_eval_device with grad f and jac g left out; the backward pass is the Lagrangian gradient
sigma grad f + J^T lambda with sigma = df, lambda = dg (zeros for an output whose gradient is None): the Jacobian never reaches memory.
All launches run on torch.cuda.current_stream().

Second derivatives in x: the Lagrangian gradient is itself a differentiable function of x whose backward pass is the Hessian-vector
product.  lagrangian_gradient(x, ...) with x.requires_grad, and loss.backward(create_graph=True) / torch.autograd.grad(...,
create_graph=True) through nlp(x), record it; without create_graph the backward pass is exactly the one launch above.  The derivatives
of the Lagrangian gradient with respect to sigma and lam are grad f . w and J w.  The engine has no fused one-launch Jacobian-vector
product for this NLP (the rows of g are not knot-local); it has the product from a stored value run of jac g.  By default a double
backward that needs them — a loss that is not linear in f and g, e.g. (f ** 2).sum(), or a sigma / lam that requires grad — raises
NotImplementedError instead of returning zeros.  KinodynamicNLP(..., jacobian_products=True) returns them through
jacobian_vector_product (two launches: evaluate grad f and jac g into memory, multiply), so that a double backward through
(f ** 2).sum() + (g ** 2).sum() runs.  No third derivative; no derivative with respect to the parameters.

The static pose finder, a batch of B independent poses, has the same interface and is complete to second order:

    nlp = PoseNLP(settings, model, batch=B)                # one pose handle (hipnlp_pose_create) on cuda:`device`
    nlp.set_params(p)                                      # [B, 202]
    f, g = nlp(x)                                          # x: [B, 81] -> f [B], g [B, m]
    gx = nlp.lagrangian_gradient(x, sigma, lam)            # ONE launch (hipnlp_pose_eval_lagrangian_grad_device)
    dot, jv = nlp.jacobian_vector_product(x, v)            # grad f . v [B], J v [B, m], ONE launch (hipnlp_pose_eval_jac_vec_device)
    hv = nlp.hessian_vector_product(x, sigma, lam, v)      # ONE launch (hipnlp_pose_eval_hess_vec_device)
    K = nlp.kkt(x, sigma, lam, dx, dc)                     # PoseKKTValues: the two value runs (two evaluation launches)
    top, bottom = K.matvec(v, w)                           # ONE launch (hipnlp_pose_kkt_times_device)
    z = K.solve(b_top, b_bottom, minv="diagonal")          # the WHOLE MINRES solve in ONE launch (hipnlp_pose_kkt_minres_device); z.status
    F = K.factor(delta_init=1e-4, kappa=8.0, max_tries=8)  # dense L D L^T per pose with F.inertia, F.status, F.delta, F.tries: ONE launch
    top, bottom = F.solve(b_top, b_bottom, refine=1)       #   (hipnlp_pose_kkt_ldl_device); solves from the stored factor (hipnlp_pose_kkt_ldl_solve_device)
    top, bottom, inertia, status = K.solve_direct(b_top, b_bottom)   # factor, inertia and solve in ONE launch, no factor stored

A pose is one workgroup, which holds all of jac g and of the Hessian in LDS: the derivatives of the Lagrangian gradient with respect to
sigma and lam, grad f . w and J w, are one launch too, so a double backward through any loss in f and g — (f ** 2).sum() + (g ** 2).sum()
— runs: H w from one launch when x needs it, grad f . w and J w from one launch when sigma or lam needs it.  Nothing raises.

Graph capture (torch.cuda.graph; the table is DESIGN.md "Graph capture", the proof tests/test_gpu_graph_replay.py).  Every method's
docstring says which of two classes it is in.  REPLAYABLE: everything reaches the kernels through pointers and by-value arguments that
no replay invalidates; the method must have run once eagerly on the handle (the engine uploads tables and allocates workspaces at first
use, and a kernel's code is loaded at its first launch — neither may happen in a capture), else it raises RuntimeError before anything
is enqueued.  NOT REPLAYABLE: raises RuntimeError while the current stream is capturing, before anything is enqueued or allocated —
above all KinodynamicNLP.__call__: the cost reducer of hipnlp_eval_device accepts a knot's partial by the launch number, which a
captured launch bakes in, so a replay could return the previous x's f.  A warmed replayable method pays one set lookup and asks torch
nothing.  torch is imported when first needed."""
import collections
import numbers

import numpy as np

from .hipnlp import HipNlp, HipPose

_FUNCTION = None
_LGRAD_FUNCTION = None
_POSE_LGRAD_FUNCTION = None

# why no backward pass is captured: nothing here proves it.  What the guard COVERS: autograd runs a backward node on the stream of its
# forward pass, so the query sees a capture only where the forward pass ran on the capturing stream.  A forward pass on another stream is
# left to torch's and the runtime's own capture errors (the engine would join a stream that is not capturing to one that is).
_NO_BACKWARD = ("no test replays a backward pass that autograd's engine enqueued (its own stream bookkeeping between the forward and the backward "
                "pass is not this library's), and a method is called replayable only where a replay test passes")
# why no launch that evaluates the model at x is captured (but hipnlp_eval_device, which has reasons of its own below)
_NO_REFERENCE = ("not proven — the launch evaluates the model at x, no CPU reference gives the bits of such a kernel, so the replay test (replays against "
                 "the eager bits AND an independent bitwise reference) cannot be run for it, and a method is called replayable only where that test passes")
_STORED = "Evaluate outside the capture and capture what runs on stored value runs (the products, the preconditioners, solve)"
# why hipnlp_eval_device is not captured: its launch number, and what the handle remembers about jac destinations
_EVAL_SEQ = ("the cost reducer of hipnlp_eval_device accepts a knot's partial by the launch number, which a captured launch bakes in, so a replay "
             "can return the previous x's f")
_EVAL_JAC = ("hipnlp_eval_device always runs its cost reducer on a captured launch number, and it stores only the varying entries of jac g into a "
             "destination the handle remembers as filled with the constant ones — a table a replay cannot consult — from a template that set_params "
             "frees")


def _torch():
    import torch
    return torch


# ---- graph capture: the two guards (module docstring; DESIGN.md "Graph capture") -----------------------------------------------------------
def _capturing():
    """is torch's current stream capturing?  A process that never initialised the device captures nothing (and must not be made to
    initialise it by this question).  torch itself, not _torch(): the tests of the argument checks stand a bare namespace in for
    _torch(), and the import is a dictionary lookup once torch is loaded."""
    import torch
    return torch.cuda.is_initialized() and torch.cuda.is_current_stream_capturing()


def _refuse(method, why, remedy):
    """a method that is NOT replayable: RuntimeError while the current stream is capturing, before anything is enqueued or allocated"""
    if _capturing():
        raise RuntimeError("%s cannot be captured into a graph (torch.cuda.graph): %s.  %s." % (method, why, remedy))


def _warm_kinds(nlp):
    """the launch kinds that have run eagerly on nlp's engine handle (the tables and workspaces are the handle's)"""
    warm = getattr(nlp, "_warm", None)
    if warm is None or warm[0] is not nlp.engine:
        warm = nlp._warm = (nlp.engine, set())
    return warm[1]


def _enter(nlp, method, *kinds):
    """a REPLAYABLE method about to launch `kinds`: the kinds that have not run eagerly on this handle yet — RuntimeError if there are any
    while the current stream is capturing.  Warmed: set lookups, no torch query."""
    warm = _warm_kinds(nlp)
    cold = tuple(k for k in kinds if k not in warm)
    if cold and _capturing():
        raise RuntimeError("%s: first use on this handle (%s) while the stream is capturing — at its first call the engine uploads its tables and allocates its "
                           "workspace, and the kernel's code is loaded, which a capture forbids.  Run %s once outside the capture; after that it is "
                           "replayable." % (method, ", ".join(k if isinstance(k, str) else " ".join(w for w in k if w) for k in cold), method))
    return cold


def _warmed(nlp, cold):
    """the launches of _enter's return value have been enqueued eagerly"""
    if cold:
        _warm_kinds(nlp).update(cold)


def _function():
    """the torch.autograd.Function (built at first use: torch is imported lazily)"""
    global _FUNCTION
    if _FUNCTION is None:
        torch = _torch()

        class NLPFunction(torch.autograd.Function):
            @staticmethod
            def forward(ctx, x, nlp):
                nlp._enter_forward()
                f = torch.empty(nlp.batch, dtype=torch.float64, device=x.device)
                g = torch.empty(nlp.batch, nlp.m, dtype=torch.float64, device=x.device)
                nlp._forward(x, f, g)
                ctx.save_for_backward(x)
                ctx.nlp = nlp
                return f, g

            @staticmethod
            def backward(ctx, df, dg):
                (x,) = ctx.saved_tensors
                nlp = ctx.nlp
                _refuse("the backward pass of nlp(x)", _NO_BACKWARD, "Run the backward pass outside the capture")
                sigma = df.to(torch.float64).contiguous() if df is not None else torch.zeros(nlp.batch, dtype=torch.float64, device=x.device)
                lam = dg.to(torch.float64).contiguous() if dg is not None else torch.zeros(nlp.batch, nlp.m, dtype=torch.float64, device=x.device)
                if torch.is_grad_enabled():   # (create_graph=True: the same launch, recorded, so that it can be differentiated in x)
                    return nlp._recorded_lgrad().apply(x, sigma, lam, nlp), None
                return nlp._launch(x, sigma, lam), None

        _FUNCTION = NLPFunction
    return _FUNCTION


def _lgrad_function():
    """the Lagrangian gradient as a torch.autograd.Function of (x, sigma, lam): its backward pass in x is the Hessian-vector product"""
    global _LGRAD_FUNCTION
    if _LGRAD_FUNCTION is None:
        torch = _torch()
        from torch.autograd.function import once_differentiable

        class LagrangianGradFunction(torch.autograd.Function):
            @staticmethod
            def forward(ctx, x, sigma, lam, nlp):
                ctx.save_for_backward(x, sigma, lam)
                ctx.nlp = nlp
                return nlp._launch(x.detach(), sigma.detach(), lam.detach())

            @staticmethod
            @once_differentiable
            def backward(ctx, w):
                x, sigma, lam = ctx.saved_tensors
                _refuse("the double backward pass of nlp(x)", _NO_BACKWARD, "Run it outside the capture")
                if ctx.nlp.jacobian_products:   # (opt-in: grad f . w and J w from a stored value run — evaluate, then multiply)
                    w = w.to(torch.float64).contiguous()
                    gx = ctx.nlp._launch_hvp(x, sigma, lam, w) if ctx.needs_input_grad[0] else None
                    gs = gl = None
                    if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
                        gs, gl = ctx.nlp.jacobian(x.detach())._launch(w, ctx.needs_input_grad[1], ctx.needs_input_grad[2])
                    return gx, gs, gl, None
                if ctx.needs_input_grad[1]:
                    raise NotImplementedError("the derivative of the Lagrangian gradient with respect to sigma is grad f . w: the engine has no "
                                              "such product (a loss that is not linear in f, or a sigma that requires grad)")
                if ctx.needs_input_grad[2]:
                    raise NotImplementedError("the derivative of the Lagrangian gradient with respect to lam is the Jacobian-vector product J w: "
                                              "the engine has none (a loss that is not linear in g, or a lam that requires grad)")
                gx = ctx.nlp._launch_hvp(x, sigma, lam, w.to(torch.float64).contiguous()) if ctx.needs_input_grad[0] else None
                return gx, None, None, None

        _LGRAD_FUNCTION = LagrangianGradFunction
    return _LGRAD_FUNCTION


def _pose_lgrad_function():
    """the pose finder's Lagrangian gradient as a torch.autograd.Function of (x, sigma, lam): its backward pass returns all three
    derivatives — H w in x (one launch), grad f . w in sigma and J w in lam (one launch for both)"""
    global _POSE_LGRAD_FUNCTION
    if _POSE_LGRAD_FUNCTION is None:
        torch = _torch()
        from torch.autograd.function import once_differentiable

        class PoseLagrangianGradFunction(torch.autograd.Function):
            @staticmethod
            def forward(ctx, x, sigma, lam, nlp):
                ctx.save_for_backward(x, sigma, lam)
                ctx.nlp = nlp
                return nlp._launch(x.detach(), sigma.detach(), lam.detach())

            @staticmethod
            @once_differentiable
            def backward(ctx, w):
                x, sigma, lam = ctx.saved_tensors
                nlp = ctx.nlp
                _refuse("the double backward pass of nlp(x)", _NO_BACKWARD, "Run it outside the capture")
                w = w.to(torch.float64).contiguous()
                gx = nlp._launch_hvp(x, sigma, lam, w) if ctx.needs_input_grad[0] else None
                gs = gl = None
                if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
                    gs, gl = nlp._launch_jvp(x, w, ctx.needs_input_grad[1], ctx.needs_input_grad[2])
                return gx, gs, gl, None

        _POSE_LGRAD_FUNCTION = PoseLagrangianGradFunction
    return _POSE_LGRAD_FUNCTION


class HessianValues:
    """The Hessian of the Lagrangian of every trajectory at one (x, sigma, lam), as the value run `values` [batch, nnz_h] of
    hipnlp_eval_hess_device (pattern: engine.hess_sparsity()); matvec(v) multiplies it by v [batch, n] in one launch
    (hipnlp_hess_times_device) — what the inner iterations of a CG solve at fixed x call."""

    def __init__(self, nlp, values):
        self.nlp, self.values = nlp, values

    def matvec(self, v):
        """H v [batch, n] (hipnlp_hess_times_device), one launch.  Graph capture: replayable after one eager call on the handle."""
        nlp = self.nlp
        nlp._check("v", v, (nlp.batch, nlp.n))
        cold = _enter(nlp, "HessianValues.matvec", "hess_times")
        out = _torch().empty_like(v, memory_format=_torch().contiguous_format)
        nlp._on_current_stream(lambda s: nlp.engine.hess_times_device(self.values.data_ptr(), v.data_ptr(), out.data_ptr(), stream=s))
        _warmed(nlp, cold)
        return out


class JacobianValues:
    """grad f and jac g of every trajectory at one x, as the tensors `grad` [batch, n] and `values` [batch, nnz] one hipnlp_eval_device
    launch wrote (pattern: engine.sparsity()); products with them are one launch each and run no knot program — what the inner
    iterations of a Krylov solve on the KKT system at fixed x call."""

    def __init__(self, nlp, grad, values):
        self.nlp, self.grad, self.values = nlp, grad, values

    def matvec(self, v):
        """J v [batch, m] (hipnlp_jac_times_device).  Graph capture: replayable after one eager call on the handle."""
        self.nlp._check("v", v, (self.nlp.batch, self.nlp.n))
        return self._launch(v, False, True)[1]

    def grad_dot(self, v):
        """grad f . v [batch].  Graph capture: replayable after one eager call on the handle.  (The dot needs a buffer of the handle's that matvec
        alone does not allocate: warm grad_dot or jvp themselves.)"""
        self.nlp._check("v", v, (self.nlp.batch, self.nlp.n))
        return self._launch(v, True, False)[0]

    def jvp(self, v):
        """(grad f . v [batch], J v [batch, m]) in one launch.  Graph capture: replayable after one eager call on the handle.  (The dot needs a
        buffer of the handle's that matvec alone does not allocate: a warmed matvec does not warm jvp.)"""
        self.nlp._check("v", v, (self.nlp.batch, self.nlp.n))
        return self._launch(v, True, True)

    def rmatvec(self, sigma, lam):
        """sigma grad f + J^T lam [batch, n] (hipnlp_jac_transpose_times_device): sigma a number or a [batch] tensor, lam [batch, m].
        Graph capture: replayable after one eager call on the handle (a number for sigma is baked into the graph: pass a tensor)."""
        nlp = self.nlp
        cold = _enter(nlp, "JacobianValues.rmatvec", "jac_transpose_times")
        sigma = nlp._sigma(sigma)
        nlp._check("lam", lam, (nlp.batch, nlp.m))
        out = _torch().empty_like(self.grad, memory_format=_torch().contiguous_format)
        nlp._on_current_stream(lambda s: nlp.engine.jac_transpose_times_device(self.values.data_ptr(), lam.data_ptr(), out.data_ptr(), grad_values_ptr=self.grad.data_ptr(),
                                                                               obj_factor_ptr=sigma.data_ptr(), stream=s))
        _warmed(nlp, cold)
        return out

    def _launch(self, v, want_dot, want_jv):
        torch, nlp = _torch(), self.nlp
        # (the kinds differ where the engine's first-use allocation does: the dot's partials are allocated the first time a dot is asked for)
        cold = _enter(nlp, "JacobianValues.%s" % ("jvp" if want_dot and want_jv else "grad_dot" if want_dot else "matvec"), ("jac_times", "dot" if want_dot else "", "jv" if want_jv else ""))
        dot = torch.empty(nlp.batch, dtype=torch.float64, device=v.device) if want_dot else None
        jv = torch.empty(nlp.batch, nlp.m, dtype=torch.float64, device=v.device) if want_jv else None
        nlp._on_current_stream(lambda s: nlp.engine.jac_times_device(self.values.data_ptr(), v.data_ptr(), jv.data_ptr() if want_jv else 0, dot.data_ptr() if want_dot else 0,
                                                                     grad_values_ptr=self.grad.data_ptr(), stream=s))
        _warmed(nlp, cold)
        return dot, jv


class KKTValues:
    """The KKT operator of an interior-point step at one (x, sigma, lam),

        K = [ H + diag dx    J^T      ]
            [ J             -diag dc  ]

    on the value runs of `hessian_values` (HessianValues or a [batch, nnz_h] tensor of hipnlp_eval_hess_device) and `jacobian_values`
    (JacobianValues or a [batch, nnz] tensor of hipnlp_eval_device), both of nlp's own handle.  dx [batch, n] and dc [batch, m] are the
    primal-dual diagonals (None: left out).  matvec(v, w) is ONE launch (hipnlp_kkt_times_device) — what the inner iterations of a Krylov
    solve on the KKT system call; with_diagonals(dx, dc) is the same operator with other diagonals, without a launch.  Not recorded by
    autograd."""

    ORDER = 189   # variables of a knot record: the order of a block of block_preconditioner()

    def __init__(self, nlp, hessian_values, jacobian_values, dx=None, dc=None):
        self.nlp = nlp
        self.hess = hessian_values.values if isinstance(hessian_values, HessianValues) else hessian_values
        self.jac = jacobian_values.values if isinstance(jacobian_values, JacobianValues) else jacobian_values
        cold = _enter(nlp, "KKTValues(...)", "hess_nnz")   # (the engine builds its Hessian tables when first asked for the pattern's size)
        nlp._check("hessian values", self.hess, (nlp.batch, nlp.engine.hess_nnz()))
        _warmed(nlp, cold)
        nlp._check("jacobian values", self.jac, (nlp.batch, nlp.engine.nnz))
        if dx is not None:
            nlp._check("dx", dx, (nlp.batch, nlp.n))
        if dc is not None:
            nlp._check("dc", dc, (nlp.batch, nlp.m))
        self.dx, self.dc = dx, dc

    def with_diagonals(self, dx=None, dc=None):
        """the operator on the same value runs with the diagonals dx [batch, n] and dc [batch, m] (None: left out); no launch"""
        return KKTValues(self.nlp, self.hess, self.jac, dx, dc)

    def matvec(self, v, w):
        """(top [batch, n], bottom [batch, m]) = K [v; w], v [batch, n], w [batch, m]; one launch.  Graph capture: replayable after one
        eager call on the handle."""
        torch, nlp = _torch(), self.nlp
        nlp._check("v", v, (nlp.batch, nlp.n))
        nlp._check("w", w, (nlp.batch, nlp.m))
        cold = _enter(nlp, "KKTValues.matvec", "kkt_times")
        top = torch.empty_like(v, memory_format=torch.contiguous_format)
        bottom = torch.empty_like(w, memory_format=torch.contiguous_format)
        nlp._on_current_stream(lambda s: nlp.engine.kkt_times_device(self.hess.data_ptr(), self.jac.data_ptr(), v.data_ptr(), w.data_ptr(), top.data_ptr(), bottom.data_ptr(),
                                                                     dx_ptr=self.dx.data_ptr() if self.dx is not None else 0,
                                                                     dc_ptr=self.dc.data_ptr() if self.dc is not None else 0, stream=s))
        _warmed(nlp, cold)
        return top, bottom

    def diagonal_preconditioner(self, floor=1e-10):
        """(top [batch, n], bottom [batch, m]), ready for solve(minv=...): top = 1 / max(|diag H + dx|, floor) and
        bottom = 1 / max(|dc + sum_e J_ie^2 top_col(e)|, floor), built on the device in ONE launch (hipnlp_kkt_diag_precond_device) from
        this operator's own value runs and diagonals — K.with_diagonals(dx, dc).diagonal_preconditioner() is the one that matches other
        diagonals.  The absolute value keeps M positive definite where H + diag dx is not.  floor > 0 keeps the reciprocals finite; its
        default is a guess nobody has tuned.  A NaN or an infinity in the value runs or diagonals comes out as NaN (solve: status 2).
        What it was measured to do: solve's docstring.  Graph capture: replayable after one eager call on the handle."""
        torch, nlp = _torch(), self.nlp
        if not (isinstance(floor, numbers.Real) and not isinstance(floor, bool) and 0.0 < floor < float("inf")):
            raise ValueError("floor: a finite real number > 0, not %r" % (floor,))
        cold = _enter(nlp, "KKTValues.diagonal_preconditioner", "kkt_diag_precond")
        top = torch.empty((nlp.batch, nlp.n), dtype=torch.float64, device=self.hess.device)
        bottom = torch.empty((nlp.batch, nlp.m), dtype=torch.float64, device=self.hess.device)
        nlp._on_current_stream(lambda s: nlp.engine.kkt_diag_precond_device(self.hess.data_ptr(), self.jac.data_ptr(), top.data_ptr(), bottom.data_ptr(),
                                                                            dx_ptr=self.dx.data_ptr() if self.dx is not None else 0,
                                                                            dc_ptr=self.dc.data_ptr() if self.dc is not None else 0, floor=float(floor), stream=s))
        _warmed(nlp, cold)
        return top, bottom

    def block_preconditioner(self, floor=1e-10):
        """KKTBlockPreconditioner: M^-1 = blockdiag_k(P_k^T L_k^-T |D_k|^-1 L_k^-1 P_k) (+) diag(top of the six globals) (+) diag(bottom),
        ready for solve(minv=...).  Graph capture: replayable after one eager call on the handle.
        TWO launches: the per-knot Bunch-Kaufman factorisation of H_k + diag dx_k (hipnlp_kkt_block_factor_device,
        one workgroup per knot and trajectory) and the diagonal launch of diagonal_preconditioner (its bottom and its six globals' top
        elements, bit for bit).  .inertia [batch, N, 3] int32 (positive, negative, zero eigenvalues of every H_k + dx_k) and .status
        [batch, N] int32 (0 factored, 2 data not finite: that knot's 189 elements come out of apply as NaN, solve: status 2); nothing is
        retried or regularised.  |D| floors every |eigenvalue| at floor > 0 (a guess nobody has tuned), so M is positive definite whatever
        the inertia.  Tied to the value runs and diagonals it was built from: K.with_diagonals(dx, dc).block_preconditioner() is the one
        that matches other diagonals.  The factor takes 143 640 B per knot and trajectory.  Measured with scipy's MINRES on the CPU (true
        relative residual 1e-8, dx and dc in U[1, 2] — not an interior-point method's, LAPACK's Bunch-Kaufman): real value runs at N = 4
        515 iterations against the diagonal's 2 425 (stairs) and 340 against 2 025 (periodic); periodic N = 10 605 where the diagonal had
        not converged at 3 000; stairs N = 10 4.8e-8 after 1 061, not 1e-8.  With the CPU emulation of these launches (rtol 1e-8 in
        the M^-1 norm): 456 against 2 194 (stairs N = 4), 315 against 1 663 (periodic N = 4).  On the device: profiles/r16_kkt_block.txt.
        NOT claimed: that an interior-point step is cheap with it; with dx, dc a factor 1e-4 smaller neither preconditioner was seen to
        converge."""
        torch, nlp = _torch(), self.nlp
        if not (isinstance(floor, numbers.Real) and not isinstance(floor, bool) and 0.0 < floor < float("inf")):
            raise ValueError("floor: a finite real number > 0, not %r" % (floor,))
        cold = _enter(nlp, "KKTValues.block_preconditioner", "kkt_block_factor", "kkt_diag_precond")
        dev, nbytes = self.hess.device, nlp.engine.kkt_block_bytes()
        N = (nlp.n - 6) // self.ORDER                                          # knots: n = 189 N + the six globals
        factor = torch.empty((nlp.batch, N, nbytes[0] // (8 * nlp.batch * N)), dtype=torch.float64, device=dev)
        pivots = torch.empty((nlp.batch, N, nbytes[1] // (4 * nlp.batch * N)), dtype=torch.int32, device=dev)
        e = torch.empty((nlp.batch, N, nbytes[2] // (8 * nlp.batch * N)), dtype=torch.float64, device=dev)
        assert factor.shape[2] == self.ORDER * (self.ORDER + 1) // 2 and pivots.shape[2] == e.shape[2] == self.ORDER
        o = torch.empty_like(e)
        inertia = torch.empty((nlp.batch, N, 3), dtype=torch.int32, device=dev)
        status = torch.empty((nlp.batch, N), dtype=torch.int32, device=dev)
        nlp._on_current_stream(lambda s: nlp.engine.kkt_block_factor_device(self.hess.data_ptr(), factor.data_ptr(), pivots.data_ptr(), e.data_ptr(), o.data_ptr(),
                                                                            inertia.data_ptr(), status.data_ptr(), dx_ptr=self.dx.data_ptr() if self.dx is not None else 0,
                                                                            floor=float(floor), stream=s))
        top, bottom = self.diagonal_preconditioner(floor)
        _warmed(nlp, cold)
        return KKTBlockPreconditioner(self, factor, pivots, e, o, inertia, status, top, bottom)

    def convexify(self, delta_init=1e-4, kappa=8.0, max_tries=16, floor=1e-10):
        """KKTBlockPreconditioner of the CONVEXIFIED operator: every knot climbs an inertia-correcting ladder on its own block until
        H_k + diag dx_k + delta_k I is positive definite, and the returned object carries the operator that goes with it.  What it does:
        (1) ONE ladder launch (hipnlp_kkt_block_ladder_device, one workgroup per knot and trajectory): try 0 is block_preconditioner's
        factorisation; try t >= 1 factors the block again, whole, with delta_t = delta_init kappa^(t-1) on its 189 diagonal elements; a
        knot stops at its first try with the inertia (189, 0, 0), or at try max_tries (0 .. 16).  (2) dx' = dx + delta_k on knot k's 189
        variables, the six globals unchanged, dx = None counting as zeros (plain torch).  (3) the diagonal launch of
        diagonal_preconditioner on K' = self.with_diagonals(dx', dc), for the bottom and the six globals.
        The result has block_preconditioner's attributes — of every knot's LAST try — and .delta [batch, N], .tries [batch, N] int32,
        .status [batch, N] (0 factored; 2 data not finite; 3 ladder exhausted: the inertia of try max_tries is stored and is not
        (189, 0, 0)), .values = K', the operator to solve on: pre.values.solve(b_top, b_bottom, minv=pre), and .quasi_definite [batch]
        bool: every knot status 0 with inertia (189, 0, 0), dx > 0 at the six globals, and dc given and > 0 everywhere.
        GUARANTEED where .quasi_definite holds and the Hessian pattern couples no two knots: the top block of .values is positive
        definite, so .values is symmetric quasi-definite with inertia exactly (n, m, 0) — the figure IPOPT's regularisation loop asks
        for — without a factorisation of K'; every pivot of the stored factors is 1x1 and positive, so apply() is the inverse of the top
        blocks of .values, not of an absolute value of them.  (A pattern with a periodicity coupling of the horizon ends has entries
        outside every block: they are in .values and in no delta_k.)
        NOT guaranteed: that delta is minimal in IPOPT's sense — this is a sufficient and conservative correction: IPOPT needs only the
        Hessian reduced to the null space of J positive definite and adds ONE delta to the whole top block, while here every knot makes
        its whole block positive definite, which can take more; nor that MINRES converges on .values, with this preconditioner or any
        other.  delta_init and kappa default to IPOPT's first_hessian_perturbation and perturb_inc_fact; nobody has tuned them here, nor
        floor.  Cost: (tries + 1) factorisations for the slowest knot of the launch; measured: profiles/r17_kkt_ladder.txt.
        max_tries = 0 is block_preconditioner with delta 0 and tries 0.  Nothing is synchronised: all attributes are device tensors.
        Graph capture: replayable whole, its torch operations included, after one eager call on the handle."""
        torch, nlp = _torch(), self.nlp
        floor = _checked_floor(floor)
        if not (isinstance(max_tries, numbers.Integral) and not isinstance(max_tries, bool) and 0 <= max_tries <= 16):
            raise ValueError("max_tries: an integer in 0 .. 16, not %r" % (max_tries,))
        if not (isinstance(delta_init, numbers.Real) and not isinstance(delta_init, bool) and 0.0 < delta_init < float("inf")):
            raise ValueError("delta_init: a finite real number > 0, not %r" % (delta_init,))
        if not (isinstance(kappa, numbers.Real) and not isinstance(kappa, bool) and 1.0 < kappa < float("inf")):
            raise ValueError("kappa: a finite real number > 1, not %r" % (kappa,))
        cold = _enter(nlp, "KKTValues.convexify", "kkt_block_ladder", "kkt_diag_precond")
        dev, nbytes = self.hess.device, nlp.engine.kkt_block_bytes()
        N = (nlp.n - 6) // self.ORDER                                          # knots: n = 189 N + the six globals
        factor = torch.empty((nlp.batch, N, nbytes[0] // (8 * nlp.batch * N)), dtype=torch.float64, device=dev)
        pivots = torch.empty((nlp.batch, N, nbytes[1] // (4 * nlp.batch * N)), dtype=torch.int32, device=dev)
        e = torch.empty((nlp.batch, N, nbytes[2] // (8 * nlp.batch * N)), dtype=torch.float64, device=dev)
        assert factor.shape[2] == self.ORDER * (self.ORDER + 1) // 2 and pivots.shape[2] == e.shape[2] == self.ORDER
        o = torch.empty_like(e)
        inertia = torch.empty((nlp.batch, N, 3), dtype=torch.int32, device=dev)
        status = torch.empty((nlp.batch, N), dtype=torch.int32, device=dev)
        delta = torch.empty((nlp.batch, N), dtype=torch.float64, device=dev)
        tries = torch.empty((nlp.batch, N), dtype=torch.int32, device=dev)
        nlp._on_current_stream(lambda s: nlp.engine.kkt_block_ladder_device(self.hess.data_ptr(), factor.data_ptr(), pivots.data_ptr(), e.data_ptr(), o.data_ptr(),
                                                                            inertia.data_ptr(), status.data_ptr(), delta.data_ptr(), tries.data_ptr(),
                                                                            dx_ptr=self.dx.data_ptr() if self.dx is not None else 0, floor=floor,
                                                                            delta_init=float(delta_init), kappa=float(kappa), max_tries=int(max_tries), stream=s))
        dx = torch.zeros((nlp.batch, nlp.n), dtype=torch.float64, device=dev) if self.dx is None else self.dx.clone()
        dx[:, :self.ORDER * N] += delta[:, :, None].expand(-1, -1, self.ORDER).reshape(nlp.batch, self.ORDER * N)   # (delta_k on knot k's 189 variables)
        convex = self.with_diagonals(dx, self.dc)
        top, bottom = convex.diagonal_preconditioner(floor)
        # (compared with numbers, not with a tensor built from a list: that is a copy from host memory, which a capture forbids)
        positive = (inertia[:, :, 0] == self.ORDER) & (inertia[:, :, 1] == 0) & (inertia[:, :, 2] == 0)
        quasi = (status == 0).all(dim=1) & positive.all(dim=1) & (dx[:, self.ORDER * N:] > 0.0).all(dim=1)
        quasi = quasi & (self.dc > 0.0).all(dim=1) if self.dc is not None else torch.zeros_like(quasi)
        _warmed(nlp, cold)
        return KKTBlockPreconditioner(convex, factor, pivots, e, o, inertia, status, top, bottom, delta=delta, tries=tries, quasi_definite=quasi)

    def condensed_preconditioner(self, floor=1e-10):
        """KKTBlockPreconditioner of the CONDENSED blocks, ready for solve(minv=...) and apply(); raises ValueError without dc.  Where
        dc > 0 the bottom block of K can be eliminated instead of approximated: C = H + diag dx + J^T diag(1 / dc) J, and by Haynsworth
        In(K) = (0, m, 0) + In(C).  C is block tridiagonal by knot; ONE launch (hipnlp_kkt_condensed_factor_device, one workgroup per knot
        and trajectory) assembles and factors its diagonal blocks B_k = H_k + diag dx_k + J_k^T diag(1 / dc) J_k from the knot's own column
        block of jac g and writes the diagonal that goes with them: .bottom = 1 / dc, .top_diagonal = 1 / max(|diag B_k|, floor) and, at
        the six globals, 1 / max(|dx_g + sum_i J_ig^2 / dc_i|, floor).  (pre.top_diagonal, pre.bottom) alone is a condensed DIAGONAL
        preconditioner for solve(minv=(top, bottom)).  M^-1 = blockdiag_k(P_k^T L_k^-T |D_k|^-1 L_k^-1 P_k) (+) that diagonal, positive
        definite whatever the inertia.  .condensed is True; the other attributes are block_preconditioner's, of the blocks B_k.
        .status [batch, N]: 0 factored; 2 block data not finite, or a dc_i of a row touching the knot's column block that is not a finite
        number > 0 (that row's .bottom is NaN); such a knot's elements come out of apply as NaN, solve: status 2.
        WHAT .inertia PROVES: every B_k is a principal submatrix of C, so a B_k with a negative (or zero) eigenvalue proves that K does NOT
        have IPOPT's inertia (n, m, 0).  All B_k positive definite proves NOTHING about K: C's off-diagonal blocks are not looked at.
        Measured with the CPU emulation (rtol 1e-8, real N = 4 value runs): 58 iterations against block_preconditioner's 315 (periodic),
        133 against 456 (stairs); with dx, dc a factor 1e-4 smaller 247 and 340 where block_preconditioner stands at status 1 after 3 000.
        On the device (profiles/r18_kkt_condensed.txt): the launch is 1.14 x block_preconditioner's factor launch, an iteration costs the
        same; at 100 x 1 and 100 x 64 (planar) every trajectory converges within 3 000 iterations at both scales (556; 282 - 1 017) where
        the block preconditioner does not; on the stairs at 200 x 16 nothing converges.  NOT claimed: convergence at other shapes or diagonals; that an interior-point
        step is cheap with it; any inertia correction (a ladder on B_k is not built); anything about the off-diagonal blocks of C — a
        block-tridiagonal factorisation would be the exact inverse of C, this is not.  Nothing is synchronised.  Graph capture: replayable
        after one eager call on the handle."""
        torch, nlp = _torch(), self.nlp
        floor = _checked_floor(floor)
        if self.dc is None:
            raise ValueError("condensed_preconditioner: the condensed block eliminates the bottom block, which needs dc > 0 — these values have no dc (with_diagonals)")
        cold = _enter(nlp, "KKTValues.condensed_preconditioner", "kkt_condensed_factor")
        dev, nbytes = self.hess.device, nlp.engine.kkt_block_bytes()
        N = (nlp.n - 6) // self.ORDER                                          # knots: n = 189 N + the six globals
        factor = torch.empty((nlp.batch, N, nbytes[0] // (8 * nlp.batch * N)), dtype=torch.float64, device=dev)
        pivots = torch.empty((nlp.batch, N, nbytes[1] // (4 * nlp.batch * N)), dtype=torch.int32, device=dev)
        e = torch.empty((nlp.batch, N, nbytes[2] // (8 * nlp.batch * N)), dtype=torch.float64, device=dev)
        assert factor.shape[2] == self.ORDER * (self.ORDER + 1) // 2 and pivots.shape[2] == e.shape[2] == self.ORDER
        o = torch.empty_like(e)
        inertia = torch.empty((nlp.batch, N, 3), dtype=torch.int32, device=dev)
        status = torch.empty((nlp.batch, N), dtype=torch.int32, device=dev)
        top = torch.empty((nlp.batch, nlp.n), dtype=torch.float64, device=dev)
        bottom = torch.empty((nlp.batch, nlp.m), dtype=torch.float64, device=dev)
        nlp._on_current_stream(lambda s: nlp.engine.kkt_condensed_factor_device(self.hess.data_ptr(), self.jac.data_ptr(), self.dc.data_ptr(), factor.data_ptr(), pivots.data_ptr(),
                                                                                e.data_ptr(), o.data_ptr(), inertia.data_ptr(), status.data_ptr(), top.data_ptr(), bottom.data_ptr(),
                                                                                dx_ptr=self.dx.data_ptr() if self.dx is not None else 0, floor=floor, stream=s))
        _warmed(nlp, cold)
        pre = KKTBlockPreconditioner(self, factor, pivots, e, o, inertia, status, top, bottom)
        pre.condensed = True
        return pre

    def solve(self, rhs_top, rhs_bottom, rtol=1e-8, maxiter=200, minv=None, check_every=16):
        """KKTSolution(top [batch, n], bottom [batch, m], iterations [batch] int32, residual [batch], status [batch] int32) of
        K [top; bottom] = [rhs_top; rhs_bottom] by preconditioned MINRES from a zero start, resident on the device
        (hipnlp_kkt_minres_device: three launches per iteration, the scalars never visit the host).  minv: a pair (top [batch, n], bottom
        [batch, m]) of positive diagonals, the preconditioner M^-1 (None: the identity), or the KKTBlockPreconditioner of
        block_preconditioner() (hipnlp_kkt_minres_block_device: the same launches, the first of every iteration with the knot's stored
        factor).  status 0: residual <= rtol, the relative
        residual in the M^-1 norm; 1: maxiter reached; 2: breakdown (minv not positive, or data that is not finite).  check_every = k > 0
        waits for the stream after every k iterations and stops once every trajectory has a status; 0 enqueues maxiter iterations
        without ever waiting — the same bits.  The solves of one nlp share a workspace: keep them on one stream.  Not recorded by
        autograd: a right-hand side that requires grad gets a solution without a graph.  No convergence is promised on the KKT systems of
        real iterates (indefinite, badly scaled).  minv=self.diagonal_preconditioner() is the one preconditioner built here; measured with
        it (rtol 1e-8, the CPU emulation of these launches, dx and dc in U[1, 2] — not an interior-point method's): symmetrically
        rescaled synthetic systems K' = S K S with cond 1e12 converge in the 23 to 25 iterations of the unscaled system where the
        identity stands at a residual of 4e-2 after 300; on the real N = 4 value runs of the stairs terrain (cond 3e9) status 0 after
        2194 iterations where the identity has residual 0.47 after 3000, on the planar terrain about a fifth fewer iterations than the
        identity's 2123.  That does not make an interior-point step cheap; larger systems: profiles/r13_kkt_precond.txt.
        Graph capture: with check_every=0 replayable after one eager call on the handle with the same kind of minv — every replay starts
        from zero (iteration 0 resets the workspace's records), whatever status the previous one or an eager solve in between left;
        the solves and replays of one nlp share the workspace, so keep them on one stream or ordered.  check_every > 0 waits for the
        stream in the middle of the launches and is refused while capturing (RuntimeError)."""
        torch, nlp = _torch(), self.nlp
        nlp._check("rhs_top", rhs_top, (nlp.batch, nlp.n))
        nlp._check("rhs_bottom", rhs_bottom, (nlp.batch, nlp.m))
        if not (isinstance(rtol, numbers.Real) and rtol >= 0.0):
            raise ValueError("rtol: a real number >= 0, not %r" % (rtol,))
        for name, k in (("maxiter", maxiter), ("check_every", check_every)):
            if not (isinstance(k, numbers.Integral) and not isinstance(k, bool) and k >= 0):
                raise ValueError("%s: an integer >= 0, not %r" % (name, k))
        mt = mb = blk = None
        if isinstance(minv, KKTBlockPreconditioner):
            if minv.nlp is not nlp:
                raise ValueError("minv: a KKTBlockPreconditioner of another nlp")
            blk, mt, mb = minv, minv.top_diagonal, minv.bottom
        elif minv is not None:
            if not (isinstance(minv, (tuple, list)) and len(minv) == 2):
                raise TypeError("minv: a pair (top [batch, n], bottom [batch, m]), a KKTBlockPreconditioner or None")
            mt, mb = minv
            nlp._check("minv top", mt, (nlp.batch, nlp.n))
            nlp._check("minv bottom", mb, (nlp.batch, nlp.m))
        if check_every > 0:
            _refuse("KKTValues.solve(check_every=%d)" % check_every, "it waits for the stream (hipStreamSynchronize) after every check_every iterations, in the middle "
                        "of the launches, which would invalidate the capture with part of the chain recorded", "Pass check_every=0: all maxiter iterations are enqueued "
                        "without a wait, a trajectory that has a status is frozen, and the bits are the same")
        cold = _enter(nlp, "KKTValues.solve", "kkt_minres_block" if blk is not None else ("kkt_minres", "minv" if mt is not None else "no minv"))
        top = torch.empty_like(rhs_top, memory_format=torch.contiguous_format)
        bottom = torch.empty_like(rhs_bottom, memory_format=torch.contiguous_format)
        iterations = torch.empty((nlp.batch,), dtype=torch.int32, device=nlp.device)
        status = torch.empty((nlp.batch,), dtype=torch.int32, device=nlp.device)
        residual = torch.empty((nlp.batch,), dtype=torch.float64, device=nlp.device)
        if blk is not None:
            nlp._on_current_stream(lambda s: nlp.engine.kkt_minres_block_device(
                self.hess.data_ptr(), self.jac.data_ptr(), blk.factor.data_ptr(), blk.pivots.data_ptr(), blk.e.data_ptr(), blk.o.data_ptr(), mt.data_ptr(), mb.data_ptr(),
                rhs_top.data_ptr(), rhs_bottom.data_ptr(), top.data_ptr(), bottom.data_ptr(), iterations.data_ptr(), residual.data_ptr(), status.data_ptr(),
                dx_ptr=self.dx.data_ptr() if self.dx is not None else 0, dc_ptr=self.dc.data_ptr() if self.dc is not None else 0, rtol=rtol, max_iterations=maxiter,
                check_every=check_every, stream=s))
            _warmed(nlp, cold)
            return KKTSolution(top, bottom, iterations, residual, status)
        nlp._on_current_stream(lambda s: nlp.engine.kkt_minres_device(
            self.hess.data_ptr(), self.jac.data_ptr(), rhs_top.data_ptr(), rhs_bottom.data_ptr(), top.data_ptr(), bottom.data_ptr(), iterations.data_ptr(),
            residual.data_ptr(), status.data_ptr(), dx_ptr=self.dx.data_ptr() if self.dx is not None else 0, dc_ptr=self.dc.data_ptr() if self.dc is not None else 0,
            minv_top_ptr=mt.data_ptr() if mt is not None else 0, minv_bottom_ptr=mb.data_ptr() if mb is not None else 0, rtol=rtol, max_iterations=maxiter,
            check_every=check_every, stream=s))
        _warmed(nlp, cold)
        return KKTSolution(top, bottom, iterations, residual, status)


KKTSolution = collections.namedtuple("KKTSolution", "top bottom iterations residual status")


class KKTBlockPreconditioner:
    """What KKTValues.block_preconditioner built: .factor [batch, N, 17955] (L and D of every knot block, packed lower triangle by columns),
    .pivots [batch, N, 189] int32 (pivot words: bits 0..15 LAPACK's ipiv, 16..23 the permutation, 24..25 the index's place in D), .e / .o
    [batch, N, 189] (|D|^-1), .inertia [batch, N, 3] int32, .status [batch, N] int32, .top_diagonal [batch, n] (used at the six globals)
    and .bottom [batch, m] (the diagonal preconditioner's).  apply(r_top, r_bottom) is ONE launch (hipnlp_kkt_block_apply_device);
    KKTValues.solve(minv=this) runs MINRES with it.  Tied to the value runs and diagonals it was built from.
    What KKTValues.convexify built has, beside these, .delta [batch, N], .tries [batch, N] int32 and .quasi_definite [batch] bool (None
    on what block_preconditioner built), and its .values is the CONVEXIFIED operator — the one to solve on with it.
    What KKTValues.condensed_preconditioner built has .condensed True (False otherwise): its records are those of the condensed blocks
    B_k = H_k + diag dx_k + J_k^T diag(1 / dc) J_k, .bottom is 1 / dc and .top_diagonal the condensed diagonal, all from one launch."""

    condensed = False   # True on what KKTValues.condensed_preconditioner built

    def __init__(self, values, factor, pivots, e, o, inertia, status, top_diagonal, bottom, *, delta=None, tries=None, quasi_definite=None):
        self.nlp, self.values = values.nlp, values
        self.factor, self.pivots, self.e, self.o, self.inertia, self.status = factor, pivots, e, o, inertia, status
        self.top_diagonal, self.bottom = top_diagonal, bottom
        self.delta, self.tries, self.quasi_definite = delta, tries, quasi_definite

    def apply(self, r_top, r_bottom):
        """(z_top [batch, n], z_bottom [batch, m]) = M^-1 [r_top; r_bottom], one launch; a knot with status 2 yields NaN for its 189 elements.
        Graph capture: replayable after one eager call on the handle."""
        torch, nlp = _torch(), self.nlp
        nlp._check("r_top", r_top, (nlp.batch, nlp.n))
        nlp._check("r_bottom", r_bottom, (nlp.batch, nlp.m))
        cold = _enter(nlp, "KKTBlockPreconditioner.apply", "kkt_block_apply")
        z_top = torch.empty_like(r_top, memory_format=torch.contiguous_format)
        z_bottom = torch.empty_like(r_bottom, memory_format=torch.contiguous_format)
        nlp._on_current_stream(lambda s: nlp.engine.kkt_block_apply_device(self.factor.data_ptr(), self.pivots.data_ptr(), self.e.data_ptr(), self.o.data_ptr(),
                                                                           self.top_diagonal.data_ptr(), self.bottom.data_ptr(), r_top.data_ptr(), r_bottom.data_ptr(),
                                                                           z_top.data_ptr(), z_bottom.data_ptr(), stream=s))
        _warmed(nlp, cold)
        return z_top, z_bottom


class PoseKKTValues:
    """The KKT operator of an interior-point step of every pose at one (x, sigma, lam),

        K = [ H + diag dx    J^T      ]
            [ J             -diag dc  ]

    on the value runs `hess` [batch, nnz_h] (hipnlp_pose_eval_hess_device) and `jac` [batch, nnz] (hipnlp_pose_eval_device) of nlp's own
    handle; dx [batch, 81] and dc [batch, m] are the primal-dual diagonals (None: left out).  A pose is one workgroup, which holds both
    runs in LDS: matvec, diagonal_preconditioner and a WHOLE solve are one launch each, with no workspace — solves on different streams
    are independent.  Not recorded by autograd."""

    MAX_ITERATIONS = 4096   # what one launch may run (hipnlp_pose_kkt_minres_device)

    def __init__(self, nlp, hess, jac, dx=None, dc=None):
        self.nlp, self.hess, self.jac = nlp, hess, jac
        nlp._check("hessian values", hess, (nlp.batch, nlp.hess_nnz))
        nlp._check("jacobian values", jac, (nlp.batch, nlp.engine.nnz))
        if dx is not None:
            nlp._check("dx", dx, (nlp.batch, nlp.n))
        if dc is not None:
            nlp._check("dc", dc, (nlp.batch, nlp.m))
        self.dx, self.dc = dx, dc

    def _diagonals(self):
        return dict(dx_ptr=self.dx.data_ptr() if self.dx is not None else 0, dc_ptr=self.dc.data_ptr() if self.dc is not None else 0)

    def with_diagonals(self, dx=None, dc=None):
        """the operator on the same value runs with the diagonals dx [batch, 81] and dc [batch, m] (None: left out); no launch"""
        return PoseKKTValues(self.nlp, self.hess, self.jac, dx, dc)

    def matvec(self, v, w):
        """(top [batch, 81], bottom [batch, m]) = K [v; w], v [batch, 81], w [batch, m]; one launch (hipnlp_pose_kkt_times_device).
        Graph capture: replayable after one eager call on the handle."""
        torch, nlp = _torch(), self.nlp
        nlp._check("v", v, (nlp.batch, nlp.n))
        nlp._check("w", w, (nlp.batch, nlp.m))
        cold = _enter(nlp, "PoseKKTValues.matvec", "kkt_times")
        top = torch.empty_like(v, memory_format=torch.contiguous_format)
        bottom = torch.empty_like(w, memory_format=torch.contiguous_format)
        nlp._on_current_stream(lambda s: nlp.engine.kkt_times_device(self.hess.data_ptr(), self.jac.data_ptr(), v.data_ptr(), w.data_ptr(), top.data_ptr(), bottom.data_ptr(),
                                                                     stream=s, **self._diagonals()))
        _warmed(nlp, cold)
        return top, bottom

    def diagonal_preconditioner(self, floor=1e-10):
        """(top [batch, 81], bottom [batch, m]), ready for solve(minv=...): top = 1 / max(|diag H + dx|, floor) (diag H = 0 where the
        pattern has no diagonal entry) and bottom = 1 / max(|dc + sum_e J_ie^2 top_col(e)|, floor), one launch
        (hipnlp_pose_kkt_diag_precond_device).  floor > 0 keeps the reciprocals finite; its default is a guess nobody has tuned.  A NaN or
        an infinity in the value runs or diagonals comes out as NaN (solve: status 2).  solve(minv="diagonal") builds the same diagonal
        inside the solve's own launch.  Graph capture: replayable after one eager call on the handle."""
        torch, nlp = _torch(), self.nlp
        floor = _checked_floor(floor)
        cold = _enter(nlp, "PoseKKTValues.diagonal_preconditioner", "kkt_diag_precond")
        top = torch.empty((nlp.batch, nlp.n), dtype=torch.float64, device=self.hess.device)
        bottom = torch.empty((nlp.batch, nlp.m), dtype=torch.float64, device=self.hess.device)
        nlp._on_current_stream(lambda s: nlp.engine.kkt_diag_precond_device(self.hess.data_ptr(), self.jac.data_ptr(), top.data_ptr(), bottom.data_ptr(), floor=floor,
                                                                            stream=s, **self._diagonals()))
        _warmed(nlp, cold)
        return top, bottom

    def solve(self, rhs_top, rhs_bottom, rtol=1e-8, maxiter=400, minv=None, floor=1e-10):
        """KKTSolution(top [batch, 81], bottom [batch, m], iterations [batch] int32, residual [batch], status [batch] int32) of
        K [top; bottom] = [rhs_top; rhs_bottom] by preconditioned MINRES from a zero start: ONE launch for the whole solve
        (hipnlp_pose_kkt_minres_device), every pose iterating in its own workgroup until it has a status.  minv: None (the identity), a
        pair (top [batch, 81], bottom [batch, m]) of positive diagonals, or the string "diagonal": diagonal_preconditioner(floor) built
        inside the same launch (the same bits as passing the pair).  status 0: residual <= rtol, the relative residual in the M^-1 norm;
        1: maxiter (at most 4096) reached; 2: breakdown (minv not positive, or data that is not finite).  Not recorded by autograd.
        Measured with the CPU emulation of this launch (rtol 1e-8, dx and dc in U[1, 2] — not an interior-point method's): the real
        value runs of three poses of each of six settings variants, cond(K) 1e3 to 5e6, converge with minv="diagonal" in 75 to 349
        iterations, all eighteen; timings: profiles/r14_pose_kkt.txt.  Graph capture: replayable after one eager call on the handle (one
        launch, no workspace, nothing carried from one solve to the next)."""
        torch, nlp = _torch(), self.nlp
        nlp._check("rhs_top", rhs_top, (nlp.batch, nlp.n))
        nlp._check("rhs_bottom", rhs_bottom, (nlp.batch, nlp.m))
        if not (isinstance(rtol, numbers.Real) and rtol >= 0.0):
            raise ValueError("rtol: a real number >= 0, not %r" % (rtol,))
        if not (isinstance(maxiter, numbers.Integral) and not isinstance(maxiter, bool) and 0 <= maxiter <= self.MAX_ITERATIONS):
            raise ValueError("maxiter: an integer in 0 .. %d (one launch runs them all), not %r" % (self.MAX_ITERATIONS, maxiter))
        floor = _checked_floor(floor)
        mt = mb = None
        build = isinstance(minv, str)
        if build:
            if minv != "diagonal":
                raise ValueError('minv: a pair (top [batch, n], bottom [batch, m]), "diagonal" or None, not %r' % (minv,))
        elif minv is not None:
            if not (isinstance(minv, (tuple, list)) and len(minv) == 2):
                raise TypeError('minv: a pair (top [batch, n], bottom [batch, m]), "diagonal" or None')
            mt, mb = minv
            nlp._check("minv top", mt, (nlp.batch, nlp.n))
            nlp._check("minv bottom", mb, (nlp.batch, nlp.m))
        cold = _enter(nlp, "PoseKKTValues.solve", ("kkt_minres", "diagonal built" if build else "minv" if mt is not None else "no minv"))
        top = torch.empty_like(rhs_top, memory_format=torch.contiguous_format)
        bottom = torch.empty_like(rhs_bottom, memory_format=torch.contiguous_format)
        iterations = torch.empty((nlp.batch,), dtype=torch.int32, device=nlp.device)
        status = torch.empty((nlp.batch,), dtype=torch.int32, device=nlp.device)
        residual = torch.empty((nlp.batch,), dtype=torch.float64, device=nlp.device)
        nlp._on_current_stream(lambda s: nlp.engine.kkt_minres_device(
            self.hess.data_ptr(), self.jac.data_ptr(), rhs_top.data_ptr(), rhs_bottom.data_ptr(), top.data_ptr(), bottom.data_ptr(), iterations.data_ptr(),
            residual.data_ptr(), status.data_ptr(), minv_top_ptr=mt.data_ptr() if mt is not None else 0, minv_bottom_ptr=mb.data_ptr() if mb is not None else 0,
            build_diagonal=build, floor=floor, rtol=float(rtol), max_iterations=int(maxiter), stream=s, **self._diagonals()))
        _warmed(nlp, cold)
        return KKTSolution(top, bottom, iterations, residual, status)


    # ---- the dense L D L^T of K per pose (hippopt_amd/csrc/pose_ldl.h): inertia, regularisation ladder, direct solves ----------------------
    MAX_TRIES, MAX_NRHS = 16, 8   # what one launch may run (hipnlp_pose_kkt_ldl_device)

    def _ladder(self, delta_init, kappa, max_tries):
        if not (isinstance(max_tries, numbers.Integral) and not isinstance(max_tries, bool) and 0 <= max_tries <= self.MAX_TRIES):
            raise ValueError("max_tries: an integer in 0 .. %d, not %r" % (self.MAX_TRIES, max_tries))
        if max_tries == 0:
            return 0.0, 0.0, 0
        if not (isinstance(delta_init, numbers.Real) and not isinstance(delta_init, bool) and 0.0 < delta_init < float("inf")):
            raise ValueError("delta_init: a finite real number > 0 with max_tries > 0, not %r" % (delta_init,))
        if not (isinstance(kappa, numbers.Real) and not isinstance(kappa, bool) and 1.0 < kappa < float("inf")):
            raise ValueError("kappa: a finite real number > 1 with max_tries > 0, not %r" % (kappa,))
        return float(delta_init), float(kappa), int(max_tries)

    def _rhs(self, rhs_top, rhs_bottom):
        """(nrhs, whether the caller's tensors have no nrhs axis)"""
        nlp = self.nlp
        flat = isinstance(rhs_top, _torch().Tensor) and rhs_top.dim() == 2
        nrhs = 1 if flat else (int(rhs_top.shape[1]) if isinstance(rhs_top, _torch().Tensor) and rhs_top.dim() == 3 else 0)
        if not 1 <= nrhs <= self.MAX_NRHS:
            raise ValueError("right-hand sides: [batch, 81] or [batch, nrhs, 81] with 1 <= nrhs <= %d" % self.MAX_NRHS)
        nlp._check("rhs_top", rhs_top, (nlp.batch, nlp.n) if flat else (nlp.batch, nrhs, nlp.n))
        nlp._check("rhs_bottom", rhs_bottom, (nlp.batch, nlp.m) if flat else (nlp.batch, nrhs, nlp.m))
        return nrhs, flat

    def _ldl(self, rhs_top, rhs_bottom, ladder, store):
        torch, nlp = _torch(), self.nlp
        delta_init, kappa, max_tries = ladder
        nrhs = 0
        top = bottom = None
        if rhs_top is not None:
            nrhs, _ = self._rhs(rhs_top, rhs_bottom)
        cold = _enter(nlp, "PoseKKTValues.%s" % ("factor" if store else "solve_direct"), ("kkt_ldl", "factor stored" if store else "solve"))
        if rhs_top is not None:
            top = torch.empty_like(rhs_top, memory_format=torch.contiguous_format)
            bottom = torch.empty_like(rhs_bottom, memory_format=torch.contiguous_format)
        dev = self.hess.device
        inertia = torch.empty((nlp.batch, 3), dtype=torch.int32, device=dev)
        status = torch.empty((nlp.batch,), dtype=torch.int32, device=dev)
        tries = torch.empty((nlp.batch,), dtype=torch.int32, device=dev)
        delta = torch.empty((nlp.batch,), dtype=torch.float64, device=dev)
        factor = pivots = None
        if store:
            factor = torch.empty((nlp.batch, nlp.engine.kkt_ldl_doubles()), dtype=torch.float64, device=dev)
            pivots = torch.empty((nlp.batch, nlp.n + nlp.m), dtype=torch.int32, device=dev)
        ptr = lambda t: t.data_ptr() if t is not None else 0  # noqa: E731
        nlp._on_current_stream(lambda s: nlp.engine.kkt_ldl_device(
            self.hess.data_ptr(), self.jac.data_ptr(), inertia.data_ptr(), status.data_ptr(), nrhs=nrhs, rhs_top_ptr=ptr(rhs_top), rhs_bottom_ptr=ptr(rhs_bottom),
            sol_top_ptr=ptr(top), sol_bottom_ptr=ptr(bottom), delta_ptr=delta.data_ptr(), tries_ptr=tries.data_ptr(), delta_init=delta_init, kappa=kappa, max_tries=max_tries,
            factor_ptr=ptr(factor), pivots_ptr=ptr(pivots), stream=s, **self._diagonals()))
        _warmed(nlp, cold)
        return top, bottom, inertia, status, delta, tries, factor, pivots

    def factor(self, delta_init=None, kappa=8.0, max_tries=0):
        """PoseKKTFactor: the dense L D L^T of K of every pose (Bunch-Kaufman pivoting, packed, in the pose's workgroup), ONE launch
        (hipnlp_pose_kkt_ldl_device), with .inertia [batch, 3] int32 (positive, negative, zero eigenvalues), .status [batch] int32
        (0 factored, 1 exactly singular, 2 data not finite, 3 ladder exhausted), .delta [batch] and .tries [batch] int32.
        max_tries = 0: factor once, report the inertia as it is.  max_tries > 0 (at most 16): IPOPT's inertia correction on the top
        block — try t >= 1 adds delta_init kappa^(t-1) to its diagonal — until the inertia is (81, m, 0).  Timings: profiles/r15_pose_ldl.txt.
        Graph capture: replayable after one eager call on the handle."""
        ladder = self._ladder(delta_init, kappa, max_tries)
        _, _, inertia, status, delta, tries, factor, pivots = self._ldl(None, None, ladder, True)
        return PoseKKTFactor(self, factor, pivots, inertia, status, delta, tries, regularised=ladder[2] > 0)

    def solve_direct(self, rhs_top, rhs_bottom, delta_init=None, kappa=8.0, max_tries=0):
        """(top, bottom, inertia [batch, 3] int32, status [batch] int32): factor (with the ladder of `factor`) and solve in ONE launch,
        no factor stored; right-hand sides [batch, 81] / [batch, m] or [batch, nrhs, 81] / [batch, nrhs, m], nrhs <= 8.  With status 1
        or 2 the solution is NaN; with a delta > 0 it is the solution of the regularised system.  Graph capture: replayable after one
        eager call on the handle."""
        ladder = self._ladder(delta_init, kappa, max_tries)
        top, bottom, inertia, status, _, _, _, _ = self._ldl(rhs_top, rhs_bottom, ladder, False)
        return top, bottom, inertia, status


class PoseKKTFactor:
    """The stored factor of PoseKKTValues.factor: .factor [batch, N (N + 1) / 2] (packed lower triangle, N = 81 + m), .pivots [batch, N]
    int32, .inertia [batch, 3], .status, .delta, .tries (device tensors; nothing is synchronised)."""

    def __init__(self, values, factor, pivots, inertia, status, delta, tries, regularised):
        self.values, self.factor, self.pivots = values, factor, pivots
        self.inertia, self.status, self.delta, self.tries = inertia, status, delta, tries
        self.regularised = regularised

    def _solve(self, rhs_top, rhs_bottom, nrhs):
        torch, nlp = _torch(), self.values.nlp
        cold = _enter(nlp, "PoseKKTFactor.solve", "kkt_ldl_solve")
        top = torch.empty_like(rhs_top, memory_format=torch.contiguous_format)
        bottom = torch.empty_like(rhs_bottom, memory_format=torch.contiguous_format)
        nlp._on_current_stream(lambda s: nlp.engine.kkt_ldl_solve_device(self.factor.data_ptr(), self.pivots.data_ptr(), nrhs, rhs_top.data_ptr(), rhs_bottom.data_ptr(),
                                                                         top.data_ptr(), bottom.data_ptr(), stream=s))
        _warmed(nlp, cold)
        return top, bottom

    def solve(self, rhs_top, rhs_bottom, refine=0):
        """(top, bottom) of K z = b from the stored factor, one launch (hipnlp_pose_kkt_ldl_solve_device); right-hand sides [batch, 81] /
        [batch, m] or [batch, nrhs, 81] / [batch, nrhs, m], nrhs <= 8.  refine = k adds k rounds of iterative refinement composed of
        existing launches: r = b - K z by the one-launch matvec (hipnlp_pose_kkt_times_device), a solve of r from the factor, z += it.
        The ladder's delta is in the FACTOR only: the values' operator has their own dx.  So where a ladder was asked for, the
        refinement runs against dx + delta — it converges to the solution of the REGULARISED system; it converges to the solution of
        the unregularised system only where delta = 0.  Graph capture: replayable, the refinement's torch operations included, after one
        eager call on the handle (with refine > 0 where the capture has it: the refinement launches the matvec too)."""
        torch, v = _torch(), self.values
        nrhs, flat = v._rhs(rhs_top, rhs_bottom)
        if not (isinstance(refine, numbers.Integral) and not isinstance(refine, bool) and refine >= 0):
            raise ValueError("refine: an integer >= 0, not %r" % (refine,))
        _enter(v.nlp, "PoseKKTFactor.solve", "kkt_ldl_solve", *(("kkt_times",) if refine else ()))   # (both, before the first launch)
        top, bottom = self._solve(rhs_top, rhs_bottom, nrhs)
        if refine:
            op = v
            if self.regularised:
                dx = self.delta[:, None].expand(v.nlp.batch, v.nlp.n)
                op = v.with_diagonals((dx if v.dx is None else v.dx + dx).contiguous(), v.dc)
            for _ in range(int(refine)):
                if flat:
                    kt, kb = op.matvec(top, bottom)
                else:
                    prods = [op.matvec(top[:, r].contiguous(), bottom[:, r].contiguous()) for r in range(nrhs)]
                    kt, kb = torch.stack([q[0] for q in prods], 1), torch.stack([q[1] for q in prods], 1)
                et, eb = self._solve((rhs_top - kt).contiguous(), (rhs_bottom - kb).contiguous(), nrhs)
                top, bottom = top + et, bottom + eb
        return top, bottom


def _checked_floor(floor):
    if not (isinstance(floor, numbers.Real) and not isinstance(floor, bool) and 0.0 < floor < float("inf")):
        raise ValueError("floor: a finite real number > 0, not %r" % (floor,))
    return float(floor)


class _DeviceNLP:
    """what the two NLPs share: an engine handle on cuda:`device_index` with batch, n, m, np; tensors checked to be float64, contiguous and
    on that device; launches ordered on torch.cuda.current_stream()"""

    @property
    def device(self):
        return _torch().device("cuda", self.device_index)

    def set_params(self, p):
        """p [batch, np] (numpy array or tensor): the parameters of every trajectory.  Graph capture: not replayable (a synchronous host
        copy), refused while capturing."""
        _refuse("set_params", "it copies from host memory and waits for the stream", "Set the parameters outside the capture")
        if hasattr(p, "detach"):
            p = p.detach().cpu().numpy()
        self.engine.set_params(np.asarray(p, dtype=np.float64))

    def _sigma(self, sigma):
        if isinstance(sigma, numbers.Real):
            sigma = _torch().full((self.batch,), float(sigma), dtype=_torch().float64, device=self.device)
        self._check("sigma", sigma, (self.batch,))
        return sigma

    def _on_current_stream(self, launch):
        """launch(stream handle), ordered on torch.cuda.current_stream().  A NULL stream means the handle's OWN stream to the library
        (include/hipnlp.h), so on torch's default stream the launch goes to a private stream that waits for the current one, and the
        current one waits for it (tensors are allocated on the current stream: nothing of it runs before the launch has ended).  That
        fork and join must never be captured (parallel branches in a graph); a capture has a stream of its own, so it never is."""
        torch = _torch()
        cur = torch.cuda.current_stream(self.device)
        if cur.cuda_stream:
            launch(cur.cuda_stream)
            return
        if _capturing():
            raise RuntimeError("a capture on the default stream: the launch would fork to the handle's side stream and join, a graph with parallel branches.  "
                               "Capture on a stream of its own (torch.cuda.graph does)")
        if getattr(self, "_side", None) is None:
            self._side = torch.cuda.Stream(device=self.device)
        self._side.wait_stream(cur)
        launch(self._side.cuda_stream)
        cur.wait_stream(self._side)

    def _check(self, name, t, shape):
        torch = _torch()
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s: a torch.Tensor, not %s" % (name, type(t).__name__))
        if t.dtype != torch.float64:
            raise TypeError("%s: dtype float64, not %s" % (name, t.dtype))
        if t.device != self.device:
            raise ValueError("%s: on %s, not %s" % (name, self.device, t.device))
        if tuple(t.shape) != tuple(shape):
            raise ValueError("%s: shape %s, not %s" % (name, tuple(shape), tuple(t.shape)))
        if not t.is_contiguous():
            raise ValueError("%s: a contiguous tensor" % name)


class KinodynamicNLP(_DeviceNLP):
    """(f, g) = nlp(x) on a [batch, n] float64 tensor of cuda:`device`, differentiable in x.  detect_simple_bounds: the reduced NLP
    (HIPNLP_FLAG_DETECT_SIMPLE_BOUNDS): g and lambda have the m rows of that problem.  jacobian_products: the recorded Lagrangian
    gradient's backward pass returns grad f . w for sigma and J w for lam (two launches: evaluate, multiply) instead of raising."""

    _recorded_lgrad = staticmethod(_lgrad_function)

    def __init__(self, settings, model, batch, device=0, detect_simple_bounds=False, jacobian_products=False):
        self.engine = HipNlp(settings, model, batch=batch, device=device, detect_simple_bounds=detect_simple_bounds)
        self.batch, self.n, self.m, self.np = self.engine.batch, self.engine.n, self.engine.m, self.engine.np
        self.device_index = int(device)
        self.jacobian_products = bool(jacobian_products)

    def __call__(self, x):
        """(f [batch], g [batch, m]); differentiable in x.  Graph capture: NOT replayable, refused while capturing (RuntimeError) — the
        launch sums f in a reducer workgroup that accepts a knot's partial by the launch number (hipnlp.hip: pub_pattern(a.seq)); a
        captured launch bakes that number in, every partial of the previous replay still carries it, and the reducer may sum the
        previous x's partials: a stale or mixed f with no error.  Its backward and double backward passes are refused too (they are
        the launches of lagrangian_gradient and hessian_vector_product, and no test replays what autograd's engine enqueues) — where
        the guard can see the capture: a backward node runs on its forward pass's stream, so that is where the forward pass ran on the
        capturing stream; with the forward pass on another stream the guard is silent and the capture error is torch's own."""
        self._check("x", x, (self.batch, self.n))
        return _function().apply(x, self)

    def _enter_forward(self):
        _refuse("KinodynamicNLP.__call__", _EVAL_SEQ, "Evaluate nlp(x) outside the capture; everything on stored value runs (jacobian(x) / hessian(...) / kkt(...) "
                     "taken outside the capture) can be captured")

    def lagrangian_gradient(self, x, sigma, lam):
        """sigma grad f(x) + J(x)^T lam per trajectory ([batch, n]): sigma a number or a [batch] tensor, lam [batch, m].
        Graph capture: NOT replayable, refused while capturing (RuntimeError) — for lack of a reference, not because anything was seen
        to go wrong: the launch evaluates the model at x, and no
        CPU reference gives the bits of such a kernel (tests/*_emu_lib.py are bitwise only for the launches on stored value runs), so the
        replay test cannot be run for it.  (Read from the code: everything reaches the kernel through pointers; the launch number
        only feeds the non-finite generation flag atomicMax(a.flag + b, a.seq), which nothing in this module reads.)"""
        torch = _torch()
        self._check("x", x, (self.batch, self.n))
        _refuse("KinodynamicNLP.lagrangian_gradient", _NO_REFERENCE, _STORED)
        if isinstance(sigma, numbers.Real):
            sigma = torch.full((self.batch,), float(sigma), dtype=torch.float64, device=self.device)
        self._check("sigma", sigma, (self.batch,))
        self._check("lam", lam, (self.batch, self.m))
        if x.requires_grad and torch.is_grad_enabled():   # (differentiable in x: the backward pass is the Hessian-vector product)
            return _lgrad_function().apply(x, sigma, lam, self)
        if self.jacobian_products and (sigma.requires_grad or lam.requires_grad) and torch.is_grad_enabled():
            return _lgrad_function().apply(x, sigma, lam, self)
        return self._launch(x, sigma, lam)

    def jacobian(self, x):
        """JacobianValues at x: one hipnlp_eval_device launch with grad f and jac g into tensors; .matvec / .grad_dot / .jvp / .rmatvec
        multiply them, one launch each.  Not recorded by autograd.  Graph capture: NOT replayable, refused while capturing (RuntimeError):
        the launch is hipnlp_eval_device, which always runs the cost reducer on a captured launch number (__call__), stores only the
        VARYING entries of jac g into a destination that the handle's own table remembers as filled with the constant ones (hipnlp.hip,
        hipnlp_eval_device: dfilled) and takes those constants from a template that set_params frees and allocates again.  Take
        jacobian(x) outside the capture; the products of the returned JacobianValues are replayable."""
        torch = _torch()
        self._check("x", x, (self.batch, self.n))
        _refuse("KinodynamicNLP.jacobian", _EVAL_JAC, "Take jacobian(x) outside the capture and capture the products on its value run")
        grad = torch.empty(self.batch, self.n, dtype=torch.float64, device=self.device)
        values = torch.empty(self.batch, self.engine.nnz, dtype=torch.float64, device=self.device)
        self._on_current_stream(lambda s: self.engine.eval_device(x.data_ptr(), 0, grad.data_ptr(), 0, values.data_ptr(), stream=s))
        return JacobianValues(self, grad, values)

    def jacobian_vector_product(self, x, v):
        """(grad f(x) . v [batch], J(x) v [batch, m]) per trajectory, v [batch, n].  TWO launches — hipnlp_eval_device writes grad f and
        jac g, hipnlp_jac_times_device multiplies them (there is no fused one-launch product for this NLP); for many products at one x
        keep jacobian(x).  Not recorded by autograd.  Graph capture: NOT replayable, refused while capturing (RuntimeError): its first
        launch is jacobian(x)'s."""
        self._check("x", x, (self.batch, self.n))
        self._check("v", v, (self.batch, self.n))
        _refuse("KinodynamicNLP.jacobian_vector_product", _EVAL_JAC, "Take J = jacobian(x) outside the capture and capture J.jvp(v)")
        return self.jacobian(x).jvp(v)

    def hessian_vector_product(self, x, sigma, lam, v):
        """H(x, sigma, lam) v per trajectory ([batch, n]), H the Hessian of sigma f + lam . g in x: sigma a number or a [batch] tensor,
        lam [batch, m], v [batch, n].  One launch; H is never written.  Not recorded by autograd.
        Graph capture: NOT replayable, refused while capturing (RuntimeError) — for lack of a reference, not because anything was seen
        to go wrong: the launch evaluates the model at x, and no
        CPU reference gives the bits of such a kernel (tests/*_emu_lib.py are bitwise only for the launches on stored value runs), so the
        replay test cannot be run for it.  (Read from the code: the launch number only feeds the non-finite generation flag, which
        nothing in this module reads.)"""
        self._check("x", x, (self.batch, self.n))
        _refuse("KinodynamicNLP.hessian_vector_product", _NO_REFERENCE, _STORED)
        sigma = self._sigma(sigma)
        self._check("lam", lam, (self.batch, self.m))
        self._check("v", v, (self.batch, self.n))
        return self._launch_hvp(x, sigma, lam, v)

    def hessian(self, x, sigma, lam):
        """HessianValues at (x, sigma, lam): one hipnlp_eval_hess_device launch; .matvec(v) is bit for bit hessian_vector_product(..., v).
        Graph capture: NOT replayable, refused while capturing (RuntimeError) — for lack of a reference, not because anything was seen
        to go wrong: the launch evaluates the model at x, and no
        CPU reference gives the bits of such a kernel (tests/*_emu_lib.py are bitwise only for the launches on stored value runs), so the
        replay test cannot be run for it.  (Read from the code: the launch number only feeds the non-finite generation flag, which
        nothing in this module reads.)  Take hessian(...) outside the capture; .matvec on it is replayable."""
        torch = _torch()
        self._check("x", x, (self.batch, self.n))
        _refuse("KinodynamicNLP.hessian", _NO_REFERENCE, _STORED)
        cold = _enter(self, "KinodynamicNLP.hessian", "hess_nnz")
        sigma = self._sigma(sigma)
        self._check("lam", lam, (self.batch, self.m))
        values = torch.empty(self.batch, self.engine.hess_nnz(), dtype=torch.float64, device=self.device)
        self._on_current_stream(lambda s: self.engine.eval_hess_device(x.data_ptr(), sigma.data_ptr(), lam.data_ptr(), values.data_ptr(), stream=s))
        _warmed(self, cold)
        return HessianValues(self, values)

    def kkt(self, x, sigma, lam, dx=None, dc=None):
        """KKTValues at (x, sigma, lam) with the diagonals dx [batch, n] and dc [batch, m] (None: left out): the two evaluation launches
        of jacobian(x) and hessian(x, sigma, lam); .matvec(v, w) applies [[H + diag dx, J^T], [J, -diag dc]] in one launch.  Not recorded
        by autograd.  Graph capture: NOT replayable, refused while capturing (RuntimeError): one of its launches is jacobian(x)'s.  Take
        kkt(...) outside the capture; everything on the returned KKTValues is replayable (solve: with check_every=0), as is
        KKTValues(nlp, H, J, dx, dc) on value runs taken outside."""
        _refuse("KinodynamicNLP.kkt", _EVAL_JAC, "Take kkt(...) outside the capture and capture what runs on it: matvec, the preconditioners, solve(check_every=0)")
        return KKTValues(self, self.hessian(x, sigma, lam), self.jacobian(x), dx, dc)

    # ---- internals ------------------------------------------------------------------------------------------------------------------
    def _forward(self, x, f, g):
        self._on_current_stream(lambda s: self.engine.eval_device(x.data_ptr(), f.data_ptr(), 0, g.data_ptr(), 0, stream=s))

    def _launch(self, x, sigma, lam):
        out = _torch().empty_like(x, memory_format=_torch().contiguous_format)
        self._on_current_stream(lambda s: self.engine.eval_lagrangian_grad_device(x.data_ptr(), sigma.data_ptr(), lam.data_ptr(), out.data_ptr(), stream=s))
        return out

    def _launch_hvp(self, x, sigma, lam, v):
        out = _torch().empty_like(x, memory_format=_torch().contiguous_format)
        self._on_current_stream(lambda s: self.engine.eval_hess_vec_device(x.data_ptr(), sigma.data_ptr(), lam.data_ptr(), v.data_ptr(), out.data_ptr(), stream=s))
        return out


class PoseNLP(_DeviceNLP):
    """(f, g) = nlp(x) of `batch` independent static poses on a [batch, 81] float64 tensor of cuda:`device`, differentiable in x to
    second order (module docstring).  Parameters are per pose: set_params takes [batch, 202]."""

    _recorded_lgrad = staticmethod(_pose_lgrad_function)

    def __init__(self, settings, model, batch, device=0):
        self.engine = HipPose(settings, model, batch=batch, device=device)
        self.batch, self.n, self.m, self.np = self.engine.batch, self.engine.n, self.engine.m, self.engine.np
        self.device_index = int(device)

    def __call__(self, x):
        """(f [batch], g [batch, m]); differentiable in x.
        Graph capture: NOT replayable, refused while capturing (RuntimeError) — for lack of a reference, not because anything was seen
        to go wrong: the launch evaluates the model at x, and no
        CPU reference gives the bits of such a kernel (tests/*_emu_lib.py are bitwise only for the launches on stored value runs), so the
        replay test cannot be run for it.  (Read from the code: a pose's workgroup sums its own f and no launch number is involved;
        nothing is allocated after hipnlp_pose_create.)  The backward and double backward passes are refused too, where their forward
        pass ran on the capturing stream (KinodynamicNLP.__call__)."""
        self._check("x", x, (self.batch, self.n))
        return _function().apply(x, self)

    def _enter_forward(self):
        _refuse("PoseNLP.__call__", _NO_REFERENCE, _STORED)

    def lagrangian_gradient(self, x, sigma, lam):
        """sigma grad f(x) + J(x)^T lam per pose ([batch, 81]): sigma a number or a [batch] tensor, lam [batch, m].  Differentiable in x,
        sigma and lam where they require grad.
        Graph capture: NOT replayable, refused while capturing (RuntimeError) — for lack of a reference, not because anything was seen
        to go wrong: the launch evaluates the model at x, and no
        CPU reference gives the bits of such a kernel (tests/*_emu_lib.py are bitwise only for the launches on stored value runs), so the
        replay test cannot be run for it."""
        torch = _torch()
        self._check("x", x, (self.batch, self.n))
        _refuse("PoseNLP.lagrangian_gradient", _NO_REFERENCE, _STORED)
        sigma = self._sigma(sigma)
        self._check("lam", lam, (self.batch, self.m))
        if (x.requires_grad or sigma.requires_grad or lam.requires_grad) and torch.is_grad_enabled():
            return _pose_lgrad_function().apply(x, sigma, lam, self)
        return self._launch(x, sigma, lam)

    def jacobian_vector_product(self, x, v):
        """(grad f(x) . v [batch], J(x) v [batch, m]) per pose, v [batch, 81].  One launch; jac g is never written.  Not recorded by autograd.
        Graph capture: NOT replayable, refused while capturing (RuntimeError) — for lack of a reference, not because anything was seen
        to go wrong: the launch evaluates the model at x, and no
        CPU reference gives the bits of such a kernel (tests/*_emu_lib.py are bitwise only for the launches on stored value runs), so the
        replay test cannot be run for it."""
        self._check("x", x, (self.batch, self.n))
        self._check("v", v, (self.batch, self.n))
        _refuse("PoseNLP.jacobian_vector_product", _NO_REFERENCE, _STORED)
        return self._launch_jvp(x, v, True, True)

    def hessian_vector_product(self, x, sigma, lam, v):
        """H(x, sigma, lam) v per pose ([batch, 81]), H the Hessian of sigma f + lam . g in x: sigma a number or a [batch] tensor,
        lam [batch, m], v [batch, 81].  One launch; H is never written.  Not recorded by autograd.
        Graph capture: NOT replayable, refused while capturing (RuntimeError) — for lack of a reference, not because anything was seen
        to go wrong: the launch evaluates the model at x, and no
        CPU reference gives the bits of such a kernel (tests/*_emu_lib.py are bitwise only for the launches on stored value runs), so the
        replay test cannot be run for it."""
        self._check("x", x, (self.batch, self.n))
        _refuse("PoseNLP.hessian_vector_product", _NO_REFERENCE, _STORED)
        sigma = self._sigma(sigma)
        self._check("lam", lam, (self.batch, self.m))
        self._check("v", v, (self.batch, self.n))
        return self._launch_hvp(x, sigma, lam, v)

    @property
    def hess_nnz(self):
        """entries of the lower triangle of the Hessian of the Lagrangian (engine.hess_sparsity())"""
        if getattr(self, "_hess_nnz", None) is None:
            self._hess_nnz = int(self.engine.hess_sparsity()[0].size)
        return self._hess_nnz

    def kkt(self, x, sigma, lam, dx=None, dc=None):
        """PoseKKTValues at (x, sigma, lam) with the diagonals dx [batch, 81] and dc [batch, m] (None: left out): two evaluation launches
        (hipnlp_pose_eval_device for jac g, hipnlp_pose_eval_hess_device) whose value runs it keeps; .matvec(v, w),
        .diagonal_preconditioner() and .solve(rhs_top, rhs_bottom) are one launch each.  Not recorded by autograd.
        Graph capture: NOT replayable, refused while capturing (RuntimeError) — for lack of a reference, not because anything was seen
        to go wrong: the launch evaluates the model at x, and no
        CPU reference gives the bits of such a kernel (tests/*_emu_lib.py are bitwise only for the launches on stored value runs), so the
        replay test cannot be run for it.  Take kkt(...) outside the capture; everything on the returned PoseKKTValues is replayable."""
        torch = _torch()
        self._check("x", x, (self.batch, self.n))
        _refuse("PoseNLP.kkt", _NO_REFERENCE, "Take kkt(...) outside the capture and capture what runs on it: matvec, diagonal_preconditioner, solve, factor, solve_direct")
        sigma = self._sigma(sigma)
        self._check("lam", lam, (self.batch, self.m))
        jac = torch.empty(self.batch, self.engine.nnz, dtype=torch.float64, device=self.device)
        hess = torch.empty(self.batch, self.hess_nnz, dtype=torch.float64, device=self.device)
        self._on_current_stream(lambda s: self.engine.eval_device(x.data_ptr(), 0, 0, 0, jac.data_ptr(), stream=s))
        self._on_current_stream(lambda s: self.engine.eval_hess_device(x.data_ptr(), sigma.data_ptr(), lam.data_ptr(), hess.data_ptr(), stream=s))
        return PoseKKTValues(self, hess, jac, dx, dc)

    # ---- internals ------------------------------------------------------------------------------------------------------------------
    def _forward(self, x, f, g):
        self._on_current_stream(lambda s: self.engine.eval_device(x.data_ptr(), f.data_ptr(), 0, g.data_ptr(), 0, stream=s))

    def _launch(self, x, sigma, lam):
        out = _torch().empty_like(x, memory_format=_torch().contiguous_format)
        self._on_current_stream(lambda s: self.engine.eval_lagrangian_grad_device(x.data_ptr(), sigma.data_ptr(), lam.data_ptr(), out.data_ptr(), stream=s))
        return out

    def _launch_jvp(self, x, v, want_dot, want_jv):
        torch = _torch()
        dot = torch.empty(self.batch, dtype=torch.float64, device=x.device) if want_dot else None
        jv = torch.empty(self.batch, self.m, dtype=torch.float64, device=x.device) if want_jv else None
        self._on_current_stream(lambda s: self.engine.eval_jac_vec_device(x.data_ptr(), v.data_ptr(), dot.data_ptr() if want_dot else 0,
                                                                          jv.data_ptr() if want_jv else 0, stream=s))
        return dot, jv

    def _launch_hvp(self, x, sigma, lam, v):
        out = _torch().empty_like(x, memory_format=_torch().contiguous_format)
        self._on_current_stream(lambda s: self.engine.eval_hess_vec_device(x.data_ptr(), sigma.data_ptr(), lam.data_ptr(), v.data_ptr(), out.data_ptr(), stream=s))
        return out
