/*
 * hipnlp.h — C-ABI of the MI355X-native multiple-shooting NLP-callback engine.
 *
 * Drop-in boundary for ONE hot path of ami-iit/hippopt: the per-knot evaluation of
 * (f, grad f, g, jac g) of the humanoid kinodynamic multiple-shooting NLP that the
 * reference assembles in
 *   src/hippopt/turnkey_planners/humanoid_kinodynamic/planner.py:26-176
 * and evaluates, through CasADi's Opti/nlpsol, once per IPOPT callback in
 *   src/hippopt/base/opti_solver.py:479   (self._solver.solve()).
 *
 * What each entry point replaces on the reference side
 *   hipnlp_create       <- cs.Opti("nlp") + opti.variable()/parameter() creation order
 *                          (base/opti_solver.py:139-175, 251-333) and the planner's
 *                          subject_to/minimize call order (planner.py:124-176)
 *   hipnlp_set_params   <- opti.set_value(parameter, value)     (opti_solver.py:236-249)
 *   hipnlp_bounds       <- Opti's canonical lbg/ubg of every subject_to
 *   hipnlp_sparsity     <- nlp_jac_g sparsity (CCS, column-major)  [CasADi, 3rd party]
 *   hipnlp_eval         <- nlp_f / nlp_grad_f / nlp_g / nlp_jac_g   [CasADi SX VM, 3rd party]
 *                          = IPOPT's eval_f / eval_grad_f / eval_g / eval_jac_g
 *                          (IpStdCInterface.h callback quartet; no eval_h: the reference
 *                          runs hessian_approximation=limited-memory,
 *                          main_periodic_step.py:116)
 *   hipnlp_eval_device  <- same, device-resident in/out (no PCIe), used by bench.py and
 *                          by the multi-GPU path (RCCL all-gather of the output shards)
 *
 * Conventions
 *   - all reals are IEEE fp64; all indices are 0-based int32
 *   - return value 0 = ok, negative = error (see HIPNLP_E_*); no exceptions cross the ABI
 *   - the caller owns every host buffer; the library owns device memory
 *   - one handle is used by one thread at a time (IPOPT is single threaded)
 *   - x, lambda order  = reference creation order: [knot 0 (189) | ... | knot N-1 | initial_state.centroidal_momentum (6)]
 *   - p order          = reference parameter creation order (tests/golden/kinodyn_structure.json)
 *   - g order          = reference subject_to call order (constraint-type-major, knot-minor)
 *   - jac order        = CCS (sorted by column, then row), fixed at create time
 */
#ifndef HIPNLP_H
#define HIPNLP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version of this header.  The caller stores it in hipnlp_desc.abi_version / hipnlp_pose_desc.abi_version; hipnlp_create and
 * hipnlp_pose_create refuse a descriptor built against another version (a C caller compiled against an older header would pass a
 * shorter struct).  History: 1 = rounds 1-2 (no version field); 2 = abi_version + flags in the descriptors, m_full / n_lifted in
 * hipnlp_dims, detect_simple_bounds layout, auto-registration, IPOPT callback quartet (hipnlp_ipopt.h); 3 = round 6:
 * hipnlp_terrain_step.top_normal (sloped step tops: the descriptors grew by 24 bytes per terrain step).                            */
#define HIPNLP_ABI_VERSION 3

#define HIPNLP_NJ 23        /* actuated joints (ergoCub: torso 3, arms 4+4, legs 6+6) */
#define HIPNLP_NL 24        /* links = root + one per joint                            */
#define HIPNLP_NC 8         /* contact points: left[0..3], right[0..3]                 */
#define HIPNLP_NXK 189      /* decision variables per knot                             */
#define HIPNLP_NPK 79       /* parameters per knot (24 descriptors + 55 references)    */
#define HIPNLP_NXG 6        /* horizon-global decision variables                       */
#define HIPNLP_NPG 326      /* horizon-global parameters                               */

/* error codes */
#define HIPNLP_OK 0
#define HIPNLP_E_INVALID (-1)   /* bad argument / inconsistent descriptor */
#define HIPNLP_E_NODEVICE (-2)  /* no HIP device / HIP runtime error      */
#define HIPNLP_E_ALLOC (-3)
#define HIPNLP_E_PARAMS (-4)    /* parameters not set before eval (opti_solver.py:447-450) */
#define HIPNLP_E_NUMERIC (-5)   /* NaN/Inf produced by the kernel (IPOPT callback must return false) */
#define HIPNLP_E_UNSUPPORTED (-6) /* the request is valid but this part is not built (hipnlp_last_error says which) */

/* ExpressionType of base/problem.py:15-19 */
#define HIPNLP_EXPR_SKIP 0
#define HIPNLP_EXPR_SUBJECT_TO 1
#define HIPNLP_EXPR_MINIMIZE 2

/* Terrain kinds.
 *   PLANAR        robot_planning/utilities/planar_terrain.py:7-41       h = p_z, n = e_z, R_t = I
 *   SMOOTH_STEPS  TerrainSum of SmoothTerrain.step bumps (utilities/smooth_terrain.py:201-227,266-336, terrain_sum.py:19-38;
 *                 the stairs of main_walking_on_stairs.py:18-28):  h = p_z - sum_s [ H_s exp(-g_s^(2 side_s)) + o_s,z ],
 *                 g_s = (2 q_x / L_s)^(2 edge_s) + (2 q_y / W_s)^(2 edge_s),  q = Rz(orientation_s)^T (p - o_s);
 *                 a step with a sloped top (hipnlp_terrain_step.top_normal):  H_s  ->  pi_s(q) = H_s - (n_x q_x + n_y q_y) / n_z;
 *                 normal / orientation from the TerrainDescriptor defaults (utilities/terrain_descriptor.py:45-80)      */
#define HIPNLP_TERRAIN_PLANAR 0
#define HIPNLP_TERRAIN_SMOOTH_STEPS 1
#define HIPNLP_MAX_TERRAIN_STEPS 4

typedef struct hipnlp_terrain_step {
    double length, width, height;
    double position[3];
    double orientation;     /* yaw of the bump (rad) */
    int32_t edge_sharpness; /* default 5  (exponent 2*edge on the footprint) */
    int32_t side_sharpness; /* default 10 (exponent 2*side on g)            */
    /* SmoothTerrain.step(top_normal_direction=...) (utilities/smooth_terrain.py:238-264; the ramp of main_walking_on_ramp.py:18-30,
     * 403-409): the top surface of the step is the plane through (0, 0, height) of the step's frame with this normal,
     *     pi(q_x, q_y) = height - (n_x q_x + n_y q_y) / n_z,   n = top_normal / |top_normal|,
     * and the bump is exp(-g^(2 side)) pi(q).  The zero vector (a zeroed struct) = the reference's None: the flat top, pi = height.
     * Refused as the reference refuses them: |top_normal| < 1e-6 (but not zero), |n_z| < 1e-6. */
    double top_normal[3];
} hipnlp_terrain_step;

/* Frame slots of hipnlp_robot_model.frame_* */
#define HIPNLP_FRAME_LEFT_SOLE 0
#define HIPNLP_FRAME_RIGHT_SOLE 1
#define HIPNLP_FRAME_CHEST 2

/*
 * Kinematic tree, adam-robotics conventions:
 *   child link of joint j is link j+1; parent[j] is ANY other link of a tree rooted at link 0 = root_link (the joint order is the
 *   reference's joints_name_list order, which fixes the x layout and need not follow the tree; chains of at most 8 joints).
 *   parent_T_child(s_j) = [ R_fix[j] * Rot(axis[j], s_j) , o_fix[j] ]   (URDF origin xyz/rpy, then axis rotation)
 *   inertials are expressed in the link frame: mass, com, 3x3 inertia about the com (row-major).
 *   frames: rigidly attached to frame_link[f] with link_T_frame = [frame_R[f], frame_o[f]].
 */
typedef struct hipnlp_robot_model {
    int32_t parent[HIPNLP_NJ];
    double R_fix[HIPNLP_NJ][9];
    double o_fix[HIPNLP_NJ][3];
    double axis[HIPNLP_NJ][3];
    double mass[HIPNLP_NL];
    double com[HIPNLP_NL][3];
    double inertia[HIPNLP_NL][9];
    int32_t frame_link[3];
    double frame_R[3][9];
    double frame_o[3][3];
} hipnlp_robot_model;

/*
 * Everything that is a python-side *setting* (a constant baked into the CasADi graph) in the
 * reference, as opposed to an Opti parameter.  Field -> reference:
 *   horizon                       settings.horizon_length                 (settings.py:19)
 *   final_state_type/weight       settings.final_state_expression_*       (planner.py:417-425)
 *   periodicity_type/weight       settings.periodicity_expression_*       (planner.py:923-930)
 *   *_multiplier / *_weights      settings.*                              (planner.py:249-264,433-520,746-895)
 *   yaw_corner[foot][0..2]        bottom-right / top-right / top-left point index per foot,
 *                                 chosen from the descriptor geometry     (planner.py:773-828)
 *   joint_reg_as_coded            1: evaluate joint_positions_error exactly as coded
 *                                 (elementwise * of a 23x23 diagonal with a 23x1 vector,
 *                                 planner.py:505-520);  0: intended sum_i (sdot_i + w_i e_i)^2
 */
typedef struct hipnlp_settings {
    int32_t horizon;
    int32_t terrain;
    int32_t final_state_type;
    int32_t periodicity_type;
    int32_t joint_reg_as_coded;
    int32_t yaw_corner[2][3];
    double final_state_weight;
    double periodicity_weight;
    double contacts_centroid_cost_multiplier;
    double com_linear_velocity_cost_weights[3];
    double com_linear_velocity_cost_multiplier;
    double desired_frame_quaternion_cost_multiplier;
    double base_quaternion_cost_multiplier;
    double base_quaternion_velocity_cost_multiplier;
    double joint_regularization_cost_weights[HIPNLP_NJ];
    double joint_regularization_cost_multiplier;
    double force_regularization_cost_multiplier;
    double foot_yaw_regularization_cost_multiplier;
    double swing_foot_height_cost_multiplier;
    double contact_velocity_control_cost_multiplier;
    double contact_force_control_cost_multiplier;
    int32_t n_terrain_steps;   /* SMOOTH_STEPS: number of bumps (1..HIPNLP_MAX_TERRAIN_STEPS) */
    int32_t reserved_;
    hipnlp_terrain_step terrain_steps[HIPNLP_MAX_TERRAIN_STEPS];
} hipnlp_settings;

typedef struct hipnlp_desc {
    hipnlp_settings settings;
    hipnlp_robot_model model;
    int32_t batch;       /* independent trajectories evaluated per call (>=1); x/p/outputs get a leading batch dim */
    int32_t knot_begin;  /* shard: this handle evaluates knots [knot_begin, knot_end) of every trajectory   */
    int32_t knot_end;    /*        (0, horizon) = whole horizon.  See DESIGN.md §6 (multi-GPU)              */
    int32_t device;      /* HIP device ordinal                                                               */
    int32_t abi_version; /* HIPNLP_ABI_VERSION of the header the caller was compiled against (checked by hipnlp_create) */
    int32_t flags;       /* HIPNLP_FLAG_*                                                                     */
} hipnlp_desc;

/* hipnlp_desc.flags
 *   DETECT_SIMPLE_BOUNDS  the handle IS the NLP nlpsol hands to IPOPT when Opti runs with {"detect_simple_bounds": True}
 *                         (main_periodic_step.py:109-110): every row of g that is exactly one decision variable — the u_v and
 *                         joint position / velocity boxes (planner.py:386-405,699-719; 70 rows per interior knot), the
 *                         `x_0 == initial_state` rows, the final-state rows that hold a variable — leaves g and jac g and becomes a
 *                         bound on that variable: m, nnz, the sparsity pattern, g, jac g, lbg / ubg and the multipliers of
 *                         hipnlp_eval_hess are those of the REDUCED problem, lbx / ubx carry the lifted bounds; the kernels never
 *                         compute or move the lifted rows.  hipnlp_lift_map relates the reduced rows to the reference's full list
 *                         of named constraints (hipnlp_row_block stays in full numbering).                                        */
#define HIPNLP_FLAG_DETECT_SIMPLE_BOUNDS 1
/*   JAC_VARYING_FIRST     order of the non-zeros of jac g INSIDE the column block of a knot (hipnlp_sparsity, every jac value array):
 *                         the entries that depend on x first (in CCS order), the constant ones behind them (in CCS order), instead of
 *                         one CCS run.  43 % of the pattern at 100 knots is constant — the +-1, -dt/2, mass entries of the trapezoid
 *                         defects (integrators/implicit_trapezoid.py:24-39), the x_0 rows (base/multiple_shooting_solver.py:713-742)
 *                         and the single-variable bound rows (planner.py:386-405,699-719) — and the host path stores only the varying
 *                         entries (hipnlp_set_constant_jacobian): in this order they are ONE contiguous run per knot on the PCIe
 *                         link instead of fragments of a few doubles.  IPOPT takes triplets in any order (eval_jac_g's structure
 *                         call), so a C binding sets the flag; a consumer that wants CasADi's CCS value array leaves it unset.
 *                         Knot blocks keep their places and sizes (shards, hipnlp_dims are unchanged).                              */
#define HIPNLP_FLAG_JAC_VARYING_FIRST 2

typedef struct hipnlp_dims {
    int32_t n;        /* decision variables per trajectory = 189*N + 6                */
    int32_t m;        /* constraint rows per trajectory                               */
    int32_t nnz;      /* structural non-zeros of jac g per trajectory                 */
    int32_t np;       /* parameters per trajectory = 79*N + 326                       */
    int32_t nnz_knot; /* non-zeros in the column block of one interior knot           */
    int32_t m_knot;   /* rows owned by one interior knot                              */
    /* shard view (== full view when the handle owns the whole horizon) */
    int32_t shard_g_rows;   /* rows written by this handle          */
    int32_t shard_nnz;      /* jac values written by this handle    */
    int32_t shard_grad;     /* grad entries written by this handle  */
    int32_t shard_jac_off;  /* offset of the handle's jac block in the CCS value array */
    int32_t shard_grad_off; /* offset of the handle's block in grad f                  */
    int32_t m_full;         /* rows of the reference's full subject_to list (== m without DETECT_SIMPLE_BOUNDS)   */
    int32_t n_lifted;       /* rows of that list that are exactly one decision variable (m_full - n_lifted = m when lifted) */
} hipnlp_dims;

typedef struct hipnlp_handle hipnlp_handle;

int hipnlp_abi_version(void);            /* HIPNLP_ABI_VERSION the library was built with */
const char* hipnlp_build_info(void);     /* how the library was built (e.g. "gfx950; ds_read2_b64 split in the assembly" or "gfx950; plain hipcc") */
/* NUMA node of the host that card `device` hangs off (-1: not known).  The host-buffer paths want the calling thread and the arrays it
 * passes on THAT node (its CPUs: /sys/devices/system/node/node<N>/cpulist): on a two-socket host the same call measured 37.6 - 39.0 us
 * with the caller pinned to the card's node and 40.2 - 41.7 us on the other one (hipnlp_eval, all four outputs, 100 knots), the exact
 * Hessian 55 against 60 - 62 us — and its early run (hipnlp_set_hessian_early_run) a gain on the card's node, a loss on the other. */
int hipnlp_device_numa_node(int device, int* node);
/* ... and the calling THREAD onto the CPUs of that node (sched_setaffinity with those of them it is allowed to run on; arrays it
 * allocates from then on follow by first touch).  node_out / cpus_out (may be NULL): the node and the number of CPUs the thread now has —
 * -1 / 0 when nothing was changed (node unknown, none of its CPUs allowed). */
int hipnlp_pin_thread_to_device_numa_node(int device, int* node_out, int* cpus_out);
int hipnlp_create(const hipnlp_desc* desc, hipnlp_handle** out);
void hipnlp_destroy(hipnlp_handle* h);
const char* hipnlp_last_error(const hipnlp_handle* h); /* h may be NULL: last create() error */
int hipnlp_get_dims(const hipnlp_handle* h, hipnlp_dims* out);

/* p: [batch][np] host array in reference parameter order. Computes bounds, uploads device copies. */
int hipnlp_set_params(hipnlp_handle* h, const double* p);

/* Canonical bounds (CasADi Opti canon form), valid after set_params.  Any pointer may be NULL.
 * lbx/ubx: [n] (+-inf: the reference adds no explicit variable bounds; with DETECT_SIMPLE_BOUNDS: the bounds of the lifted rows)
 * lbg/ubg: [m] of trajectory 0 (bounds depend on parameters only)                              */
int hipnlp_bounds(const hipnlp_handle* h, double* lbx, double* ubx, double* lbg, double* ubg);

/* is_simple[m_full]: 1 where row i of the FULL subject_to list is exactly one decision variable (what nlpsol's
 * detect_simple_bounds lifts, main_periodic_step.py:110); var_index[m_full]: that variable or -1. */
int hipnlp_simple_rows(const hipnlp_handle* h, int32_t* is_simple, int32_t* var_index);
/* The handle's rows against the reference's full list of named constraints (hipnlp_row_block): kept_row[m_full] = row of this
 * handle's g behind full row r, or -1 when the row was lifted into a bound (identity without DETECT_SIMPLE_BOUNDS);
 * lb_full / ub_full [m_full] = canonical bounds of every full row (valid after set_params).  What a binding needs to hand
 * IPOPT's multipliers back per named constraint (Output.constraint_multipliers, opti_solver.py:530-537): lambda of a kept row is
 * lambda[kept_row]; the multiplier of a lifted row is the bound multiplier z_U - z_L of its variable (hipnlp_simple_rows), given
 * to the row whose bound is the active one.  Any pointer may be NULL. */
int hipnlp_lift_map(const hipnlp_handle* h, int32_t* kept_row, double* lb_full, double* ub_full);

/* CCS pattern as triplets sorted by (col,row): irow[nnz], jcol[nnz] (IPOPT eval_jac_g, values==NULL call).
 * With HIPNLP_FLAG_JAC_VARYING_FIRST: knot blocks in knot order, inside a block the varying entries (col,row)-sorted, then the constant ones. */
int hipnlp_sparsity(const hipnlp_handle* h, int32_t* irow, int32_t* jcol);
/* mask[nnz] (order of hipnlp_sparsity): 1 where the entry of jac g does not depend on x (its value is a function of the parameters:
 * +-1, -dt/2, the mass, +-1/4), 0 elsewhere. */
int hipnlp_jac_constant_mask(const hipnlp_handle* h, unsigned char* mask);

/* Host-buffer callback quartet (IPOPT eval_f/eval_grad_f/eval_g/eval_jac_g in one fused launch).
 * x: [batch][n]; f: [batch]; grad_f: [batch][n]; g: [batch][m]; jac: [batch][nnz].  Any output may be NULL.
 * new_x = 0 lets the library return cached results of the previous evaluation (IPOPT's flag); new_x < 0 = "unknown": the library
 * compares x with its staging copy of the previous evaluation (what a binding without IPOPT's flag — cyipopt, SciPy — passes).
 *
 * What crosses PCIe (the non-NULL outputs are the call's WANT MASK): a new evaluation copies x into a pinned staging block the
 * kernel reads directly, evaluates all four outputs in ONE launch and lets the kernel store the wanted ones — plus the handle's
 * prefetch set — straight into a pinned output block (no copy command, no second staging copy); the others stay in HBM and are
 * fetched by one asynchronous copy if a later call with new_x = 0 asks for them.  An eval_g at a line-search trial point therefore
 * moves 0.2 MB, not the 1.1 MB of jac g.  Returns HIPNLP_E_NUMERIC when the evaluation produced a NaN/Inf — AFTER filling the
 * outputs (IPOPT's callback returns false; the reference hands CasADi's NaNs to IPOPT, which cuts the step).                    */
int hipnlp_eval(hipnlp_handle* h, const double* x, int new_x,
                double* f, double* grad_f, double* g, double* jac);

#define HIPNLP_WANT_F 1u
#define HIPNLP_WANT_GRAD 2u
#define HIPNLP_WANT_G 4u
#define HIPNLP_WANT_JAC 8u
#define HIPNLP_WANT_ALL 15u
/* Same evaluation, zero-copy: returns pointers INTO the library's pinned output block (valid until the next call on the handle)
 * for the outputs named in `want` (HIPNLP_WANT_*), NULL for the others.  What a binding that must copy anyway (cyipopt copies the
 * callback's return value into IPOPT's array) uses to avoid a second copy.                                                      */
int hipnlp_eval_pinned(hipnlp_handle* h, const double* x, int new_x, unsigned want,
                       const double** f, const double** grad_f, const double** g, const double** jac);
/* Outputs every NEW evaluation brings to the host besides the ones its call asks for.  Default F | GRAD | G (0.37 MB at 100 knots:
 * +7 us): IPOPT asks for f and g at every trial point and for grad f and jac g (new_x = 0) only at accepted ones.
 * HIPNLP_WANT_ALL makes every new evaluation move everything (one launch, no second round trip for jac g).                      */
int hipnlp_set_prefetch(hipnlp_handle* h, unsigned mask);
/* Constant entries of jac g on the host path (ON by default; takes effect on handles created with HIPNLP_FLAG_JAC_VARYING_FIRST only: in
 * CCS order the varying entries of a block are fragments of one to four doubles, and storing fragments over PCIe measured slower than
 * storing everything).  A HOST destination of the Jacobian values — the library's pinned block, or
 * a caller array inside a registered range (hipnlp_host_register / auto-registration) — is filled with the constant entries ONCE per
 * parameter set (the pinned block when a launch first needs it, a caller array at its first use and again after hipnlp_set_params);
 * the kernel then stores the entries that depend on x only: 628 KB instead of 1.1 MB per 100-knot Jacobian on a path that is bound by
 * the bytes crossing PCIe.  What the caller gets is the complete value array, every call.  Contract for a REGISTERED caller array: the
 * caller does not write into it between calls (IPOPT's TNLPAdapter never touches its jac_g_ buffer).  A caller that does anyway is
 * covered by a spot check — sixteen constant entries spread over the array, its first and its last among them, are compared before every
 * such launch and the array is re-filled when one differs (hipnlp_host_stats out[5] counts these) — not by a guarantee: a caller
 * that edits single entries of a registered Jacobian array must turn this off.  Arrays that are NOT registered always receive complete
 * values by a copy out of the pinned block.
 * Device-resident outputs (hipnlp_eval_device): a jac_dev buffer is filled with the constant entries at its first
 * sight and again after hipnlp_set_params (one small launch on the call's stream, in front of the evaluation); the evaluations store the
 * varying entries of every knot block only — one run in the varying-first order, scattered over the block in CasADi's CCS order (on = 1
 * on a handle WITHOUT HIPNLP_FLAG_JAC_VARYING_FIRST asks for exactly this: device destinations only, host destinations of a CCS handle keep
 * receiving every entry) — and no longer stage the constants in LDS at all.  Same contract — the caller does not write into
 * the buffer between calls — and the launch itself samples it: the one workgroup per trajectory that sums the cost compares constant
 * entries of every knot block with the handle's templates — four positions per block (its first, its last, two in between), two of them
 * per launch, alternating with the launches INTO THAT BUFFER — and puts the constants of all the trajectory's blocks back when one differs (hipnlp_host_stats out[7] counts
 * such repairs).  A sample, not a guarantee: constants
 * overwritten elsewhere in a block are returned as they are.  The record "this buffer holds the constants" is keyed by the buffer's
 * ADDRESS: a caller that frees a jac buffer and later hands over other memory at the same address (a caching allocator does that) must
 * call hipnlp_forget_jac_destination first — the next evaluation then fills the buffer again.
 * hipnlp_eval_device_shard / _peers are not affected: every entry is stored.
 * on = 0: every launch stores every entry (the behaviour of ABI 2 libraries before this switch existed).
 * Default: on for handles created with HIPNLP_FLAG_JAC_VARYING_FIRST, off for handles in CCS order. */
int hipnlp_set_constant_jacobian(hipnlp_handle* h, int on);
/* Forget that the jac destination at address p (device buffer of hipnlp_eval_device, or registered host array of hipnlp_eval) holds this
 * handle's constant entries; p = NULL: every destination the handle remembers.  The next evaluation into it fills the constants again.
 * For callers whose allocator may hand out the same address for a new buffer.  Returns the number of records dropped (>= 0), or an
 * error code (< 0).  Host arrays need no such call since ABI-compatible revision 5: their record is tied to the array's REGISTRATION
 * (hipnlp_host_register / auto-registration), and an array that was unregistered — by anybody — is filled again when it comes back. */
int hipnlp_forget_jac_destination(hipnlp_handle* h, const void* p);
/* Early outputs (opt-in, off by default).  on = 1: a NEW evaluation stores g and jac g — when its call does NOT ask for them —
 * straight into the REGISTERED caller arrays (hipnlp_host_register, or registered by the handle itself) that earlier calls passed
 * for them, before the caller asks.  IPOPT's sequence eval_f(new x), eval_g, eval_grad_f, eval_jac_g then costs one launch that moves
 * everything and calls that return at once (grad f comes from the pinned block: one 151 KB host copy), instead of a second 1.1 MB
 * transfer when the Jacobian is asked for; a rejected line-search trial point pays for a Jacobian it never reads.
 * Contract: the contents of such a g / jac array are overwritten by every new_x call on the handle from the moment the array has been
 * passed once.  That is safe for arrays the caller treats as scratch and re-reads right after the callback that fills them — IPOPT's
 * TNLPAdapter evaluates g and the Jacobian values into buffers of its own (full_g_, jac_g_) and copies out of them.  It is NOT safe
 * for grad f under IPOPT: the adapter hands eval_grad_f the storage of IPOPT's own gradient vector, which stays alive (as the
 * gradient at the current iterate) while trial points are evaluated — so grad f is excluded unless the caller asks for it with
 * on = 2, which is for callers whose grad array is scratch of their own too (hippopt_amd's HipNlpSolver callback cache).
 * A cached call (new_x = 0) that passes a DIFFERENT array for such an output re-evaluates. */
int hipnlp_set_early_outputs(hipnlp_handle* h, int on);
/* Bracket host-path launches with HIP events (for hipnlp_last_kernel_ms); off by default: an event pair costs microseconds. */
int hipnlp_set_host_timing(hipnlp_handle* h, int on);
/* Wall clock (us) of the last hipnlp_eval on the host side: us[0] staging copy of x, us[1] enqueue (launch call), us[2] waiting for
 * the GPU (kernel + its PCIe stores), us[3] copies into caller arrays that are not registered.  Diagnostic. */
int hipnlp_host_breakdown(const hipnlp_handle* h, double* us /*[4]*/);
/* Caller-owned host arrays as DIRECT kernel outputs: register the array once (page-locks it; dev_ptr, optional, receives its
 * device-visible address).  From then on a grad_f / g / jac pointer of hipnlp_eval that lies inside a registered range is stored
 * to by the kernel itself — no staging copy at all (IPOPT's TNLP adapter keeps its g and jac-value arrays for the whole solve: the
 * binding registers them at the first callback).  The device-visible address can also be passed to hipnlp_eval_device as
 * grad_dev / g_dev / jac_dev.  Also how several processes share ONE host buffer (a shared-memory segment mapped and registered by
 * each: hippopt_amd/sharded.py HostSink).  Process-wide (no handle); the caller unregisters before freeing the memory.           */
int hipnlp_host_register(void* p, size_t bytes, void** dev_ptr);
int hipnlp_host_unregister(void* p);
/* Auto-registration (ON by default): a grad_f / g / jac array (hipnlp_eval) or Hessian-value array (hipnlp_eval_hess) of at least 64 KB
 * that the call sees at the same address on two
 * CONSECUTIVE calls is registered by the handle itself (as hipnlp_host_register would) and is a direct kernel output from then on —
 * a plain binding that simply passes IPOPT's arrays gets the fast path without knowing about it.  Safety: a registration pins the
 * PAGES behind an address; should the caller free the array and the allocator map other pages at the same address, the kernel's
 * stores would go to the old pages.  Every use of an auto-registered array is therefore verified: the call writes a word of its own
 * into the first and the last entry before the evaluation and finds both overwritten afterwards (every entry of every output is
 * written by every evaluation) — if not, the range is dropped, the address is left alone from then on and the call is served through
 * the pinned block as for any unregistered array.  The check covers every pointer into a range that ANY handle of the process registered
 * by itself (the table of ranges is process wide).  At most six ranges per handle (the oldest one that the call in progress does not use
 * goes first); all are released by hipnlp_destroy or hipnlp_set_auto_register(h, 0).  Arrays registered explicitly with
 * hipnlp_host_register are the caller's responsibility and are not verified; registering an array a handle had registered by itself
 * replaces that registration with a fresh one. */
int hipnlp_set_auto_register(hipnlp_handle* h, int on);
/* Releases every range that handles of this process registered by themselves (returns how many); the handles register their arrays
 * again when they next see them twice in a row.  For a caller about to free arrays it passed to hipnlp_eval: memory that is freed while
 * a registration of it is alive and then handed out again by the allocator confuses the HIP runtime — a hipMemcpy from such memory is
 * refused with "invalid argument", or goes through the dead mapping and ends in an illegal memory access (the library's own copies
 * release the ranges that overlap their host buffer before they copy, and all of them and retry after an "invalid argument"). */
int hipnlp_host_release_auto_ranges(void);
/* Counters of the host-buffer path: out[0] arrays auto-registered so far, out[1] stale-mapping fallbacks, out[2] ranges currently
 * auto-registered, out[3] evaluations so far (kernel launches), out[4] caller arrays filled with the constant Jacobian entries so far,
 * out[5] of which re-fills after a failed spot check, out[6] constant entries of the handle's pattern, out[7] wave slices of constants
 * the kernels put back into device buffers the caller had written over (read from the device: the call waits for a small copy). */
int hipnlp_host_stats(const hipnlp_handle* h, long* out /*[8]*/);


/* Exact Hessian of the Lagrangian  sigma f(x) + lambda^T g(x)  of the kinodynamic NLP — IPOPT's eval_h (IpStdCInterface.h:
 * Eval_H_CB(n, x, new_x, obj_factor, m, lambda, new_lambda, nele_hess, iRow, jCol, values, ud)); what CasADi's nlp_hess_l
 * computes for the reference when a script does not set `hessian_approximation = limited-memory` (SURVEY 8f rank 1;
 * opti_solver.py:123-125,479).  Lower triangle (irow >= jcol) as triplets with a fixed pattern: the Hessian is block diagonal
 * by knot (the trapezoid defects are sums of one-knot terms), plus the 84 entries coupling the last knot with the first when
 * the periodicity expression is a cost.  Order: knot blocks in knot order, each sorted by (column, row), then the coupling.
 * Both terrains (1539 triplets per knot on the planar terrain, 1878 on the smooth steps, whose contact rows need the bump sum to
 * fourth order: truncated Taylor polynomials, knot_hess_terrain.h).
 *   hipnlp_hess_nnz / _sparsity   structure (the `values == NULL` call of eval_h); a shard handle reports its own knots' blocks
 *   hipnlp_eval_hess              host buffers: x [batch][n], obj_factor [batch], lambda [batch][m] -> values [batch][nnz_h]
 *                                 (a `values` array inside a range registered with hipnlp_host_register is written by the kernel
 *                                 directly: 70 instead of 113 us per 100-knot call)
 *   hipnlp_eval_hess_device       device pointers, enqueued on `stream`, not synchronised                                   */
int hipnlp_hess_nnz(hipnlp_handle* h, int64_t* nnz_h);
int hipnlp_hess_sparsity(hipnlp_handle* h, int32_t* irow, int32_t* jcol);
int hipnlp_eval_hess(hipnlp_handle* h, const double* x, const double* obj_factor, const double* lambda, double* values);
/* The same with IPOPT's new_x flag (Eval_H_CB: FALSE when x is the x of the evaluation callbacks before it — the case at every accepted
 * iterate): new_x = 0 = the x of the previous host-buffer call on this handle (hipnlp_eval*, hipnlp_eval_hess*) — its staged copy is
 * used, no host copy of x in front of the launch; new_x < 0 = unknown (compared); anything else, or nothing staged yet: x is copied.
 * new_x = 0 is a statement about THIS handle: the callbacks at x ran on it.  (Sixty-four words of x are compared with the staged copy
 * all the same and a differing sample stages x: a binding that runs the callbacks on another handle gets the right Hessian, not a stale one.)
 * hipnlp_eval_hess is new_x = 1; hipnlp_ipopt_eval_h passes IPOPT's flag. */
int hipnlp_eval_hess_at(hipnlp_handle* h, const double* x, int new_x, const double* obj_factor, const double* lambda, double* values);
/* hipnlp_eval_hess* into host memory: the run at the start of every knot block (the point columns: a quarter of the values on the planar
 * terrain, two fifths on the smooth steps) is final long before the program ends and can leave then — the same kernel, the same values,
 * bit for bit.  Whether that is FASTER is a property of the host: measured 4 - 7 us sooner per 100-knot Hessian with the calling thread on
 * the card's NUMA node (hipnlp_pin_thread_to_device_numa_node) and 2 - 3 us later from the other socket of the same box.  mode 1 / 0: on / off;
 * -1 (the default): decided once, by the handle's first Hessian call, without a clock wherever the host says enough — off when the
 * handle's launches cannot send a run ahead at all (long launches on the compact layout), on when the calling thread runs on the card's
 * NUMA node (sysfs), off when it runs on another one — the same choice in every run on the same host; only where the topology is not
 * known (one-node hosts, containers) does the handle try both on its own first calls (three to warm up, nine of each kind alternating,
 * launch to completion on the host's clock) and keep the kind with the lower MEDIAN.  Setting a mode starts that over.
 * hipnlp_get_hessian_early_run: the mode, what is in use (-1: not decided yet) and — measured choices only — the two medians in
 * microseconds (0: not measured); hipnlp_hessian_early_run_reason: one sentence on how the choice was made. */
int hipnlp_set_hessian_early_run(hipnlp_handle* h, int mode);
int hipnlp_get_hessian_early_run(const hipnlp_handle* h, int* mode, int* chosen, double* us_off, double* us_on);
const char* hipnlp_hessian_early_run_reason(const hipnlp_handle* h);
int hipnlp_eval_hess_device(hipnlp_handle* h, const double* x_dev, const double* obj_factor_dev, const double* lambda_dev,
                            double* values_dev, void* stream);
/* Device-resident variant: all pointers are device pointers on desc.device (or device-visible addresses of registered host
 * memory, hipnlp_host_register), same shapes.  Work is enqueued on `stream` (a hipStream_t passed as void*; NULL = the handle's
 * own non-blocking stream — NOT the legacy default stream: order other work against it with an explicit stream) and NOT
 * synchronised.  Launches of ONE handle must not overlap on the device (one stream at a time, or ordered streams), and a launch is
 * not replayable from a captured hipGraph: every launch carries its own sequence number, which tags the cost partials the launch's
 * reducer workgroup waits for and the non-finite flag. */
int hipnlp_eval_device(hipnlp_handle* h, const double* x_dev,
                       double* f_dev, double* grad_dev, double* g_dev, double* jac_dev,
                       void* stream);

/* Gradient of the Lagrangian  out = obj_factor grad f(x) + J(x)^T lambda,  per trajectory: the vector a device-side consumer of a batch
 * needs to differentiate a scalar built from f and g (a training loss over the trajectories, a penalty or augmented-Lagrangian merit, the
 * backward pass of hippopt_amd.autograd).  Shapes and stream rules of hipnlp_eval_hess_device: x_dev [batch][n], obj_factor_dev [batch],
 * lambda_dev [batch][m] (m of THIS handle: the reduced rows of a HIPNLP_FLAG_DETECT_SIMPLE_BOUNDS handle), out_dev [batch][n]; device
 * pointers, enqueued on `stream` (NULL = the handle's own), not synchronised.  ONE launch: every knot sums the columns of its own block
 * of jac g — 189 doubles leave per knot instead of the 1 849 of f, grad f, g and jac g; no value of jac g reaches memory.
 * Each column is summed in (column, row) order whatever the handle's jac order: CCS and varying-first handles give the same bits.  A
 * NaN / Inf in the result raises the handle's non-finite flag, as hipnlp_eval_device does.
 * Returns HIPNLP_E_PARAMS before hipnlp_set_params; HIPNLP_E_UNSUPPORTED on a multi-device handle and on a shard handle (knot_begin /
 * knot_end not the whole horizon), hipnlp_last_error says which. */
int hipnlp_eval_lagrangian_grad_device(hipnlp_handle* h, const double* x_dev, const double* obj_factor_dev, const double* lambda_dev,
                                       double* out_dev, void* stream);

/* Hessian of the Lagrangian times a vector  out = H(x, obj_factor, lambda) v,  per trajectory: the second-order object a device-side
 * consumer needs (a Newton-CG or truncated-Newton step, a gradient penalty, a Lanczos estimate of curvature, the double backward of
 * hippopt_amd.autograd).  Shapes and stream rules of hipnlp_eval_hess_device: x_dev, v_dev, out_dev [batch][n], obj_factor_dev [batch],
 * lambda_dev [batch][m] (m of THIS handle: the reduced rows of a HIPNLP_FLAG_DETECT_SIMPLE_BOUNDS handle); device pointers, enqueued on
 * `stream` (NULL = the handle's own), not synchronised.  ONE launch, H is never written: the Hessian is block diagonal by knot, every
 * knot's workgroup runs the Hessian program and sums its 189 variables over the entries it holds in LDS — 189 doubles
 * leave per knot instead of 1 539 / 1 878; the six horizon-global elements of out are zero.  Every element of out is written exactly once.
 * Each variable is summed in a fixed order (knot_hvp.h): the same bits at every position of a batch, for every jac order, and as
 * hipnlp_hess_times_device on the values of hipnlp_eval_hess_device.  out_dev may NOT alias v_dev or x_dev (other knots' workgroups read
 * them).  A NaN / Inf in the result raises the handle's Hessian non-finite flag, as hipnlp_eval_hess_device does.
 * Returns HIPNLP_E_PARAMS before hipnlp_set_params; HIPNLP_E_UNSUPPORTED on a multi-device handle and on a shard handle (knot_begin /
 * knot_end not the whole horizon: the periodicity coupling needs both horizon ends), hipnlp_last_error says which. */
int hipnlp_eval_hess_vec_device(hipnlp_handle* h, const double* x_dev, const double* obj_factor_dev, const double* lambda_dev,
                                const double* v_dev, double* out_dev, void* stream);
/* out = H v from a value run values_dev [batch][nnz_h] that hipnlp_eval_hess_device of the SAME handle wrote: for many products at one x
 * (the inner iterations of a CG solve).  No x, no parameters, no multipliers; v_dev, out_dev [batch][n], out_dev may not alias v_dev;
 * stream rules and error codes as above (no HIPNLP_E_PARAMS).  Order and arithmetic are those of hipnlp_eval_hess_vec_device: bit for
 * bit its result.  Replayable from a captured graph after one eager call on the handle (tests/test_gpu_graph_replay.py). */
int hipnlp_hess_times_device(hipnlp_handle* h, const double* values_dev, const double* v_dev, double* out_dev, void* stream);

/* Products with a STORED value run of jac g, for many products at one x (the inner iterations of a Krylov solve on the KKT system): no
 * knot program runs, no x, no parameters, no non-finite flag.  jac_values_dev [batch][nnz] is a jac run exactly as hipnlp_eval_device
 * of THIS handle leaves it — in its order (CCS or HIPNLP_FLAG_JAC_VARYING_FIRST), every entry valid, the constant ones included;
 * grad_values_dev [batch][n] the grad f of the same call.  Device pointers, enqueued on `stream` (NULL = the handle's own), not
 * synchronised; stream rules and error codes of hipnlp_hess_times_device (no HIPNLP_E_PARAMS).  Every sum runs in a fixed order from a
 * table ("The Jacobian's rows are not knot-local"): the same bits at every position of a batch and for both jac orders.
 *
 * hipnlp_jac_times_device:  jv_dev [batch][m] = J v  and / or  dot_dev [batch] = grad f . v,  v_dev [batch][n].  Either output may be
 * NULL (it is left alone), not both; dot_dev needs grad_values_dev (otherwise grad_values_dev may be NULL).  Every row of g has one
 * owner knot whose workgroup sums it from +0.0 in ascending column, one fused multiply-add per entry; every element of jv is written
 * exactly once.  grad f . v: the products of a knot summed in a fixed tree into a per-knot partial (a workspace of the handle: calls
 * that ask for dot_dev on ONE handle must be ordered on one stream), the partials added in ascending knot order by a second small
 * launch on the same stream.  The outputs may not alias the inputs.
 *
 * hipnlp_jac_transpose_times_device:  out_dev [batch][n] = obj_factor grad f + J^T lambda,  lambda_dev [batch][m]; with
 * grad_values_dev NULL (obj_factor_dev may then be NULL too)  out = J^T lambda.  One column per thread in the (column, row) order of
 * hipnlp_eval_lagrangian_grad_device, obj_factor grad f_c first (+0.0 without a gradient).
 *
 * Return HIPNLP_E_INVALID for a missing required pointer, HIPNLP_E_UNSUPPORTED on a multi-device handle, on a shard handle (knot_begin /
 * knot_end not the whole horizon) and for a layout whose tables exceed what the kernels stage (hipnlp_last_error says which).
 * Both: replayable from a captured graph after one eager call on the handle — for hipnlp_jac_times_device an eager call WITH dot_dev where the captured one
 * has it: the dot's partials are allocated the first time a dot is asked for (tests/test_gpu_graph_replay.py). */
int hipnlp_jac_times_device(hipnlp_handle* h, const double* jac_values_dev, const double* grad_values_dev, const double* v_dev,
                            double* jv_dev, double* dot_dev, void* stream);
int hipnlp_jac_transpose_times_device(hipnlp_handle* h, const double* jac_values_dev, const double* grad_values_dev,
                                      const double* obj_factor_dev, const double* lambda_dev, double* out_dev, void* stream);

/* The KKT operator of an interior-point step, applied to a vector, from STORED value runs — the object a Krylov solve on the KKT system at
 * a fixed x multiplies by, in ONE launch instead of hipnlp_hess_times_device + hipnlp_jac_times_device +
 * hipnlp_jac_transpose_times_device and the element-wise kernels between them:
 *
 *     top_dev    [batch][n] = (H + diag d_x) v + J^T w
 *     bottom_dev [batch][m] =  J v - diag(d_c) w
 *
 * hess_values_dev [batch][nnz_h] is a run as hipnlp_eval_hess_device of the SAME handle wrote it (H = H(x, obj_factor, lambda) of that
 * call), jac_values_dev [batch][nnz] a jac run as hipnlp_eval_device of the same handle wrote it (its order, CCS or
 * HIPNLP_FLAG_JAC_VARYING_FIRST, the constant entries included).  v_dev, dx_dev, top_dev [batch][n]; w_dev, dc_dev, bottom_dev [batch][m]
 * (m of THIS handle: the reduced rows of a HIPNLP_FLAG_DETECT_SIMPLE_BOUNDS handle).  dx_dev and dc_dev are the primal-dual diagonals
 * (Sigma + delta_x and delta_c): they change between solves at one x and are arguments of every call; either may be NULL (that term is
 * left out, nothing is read).  No knot program runs: no x, no parameters, no non-finite flag.  Device pointers, enqueued on `stream`
 * (NULL = the handle's own), not synchronised; stream rules of hipnlp_hess_times_device.  The outputs may not alias the inputs.
 *
 * Order of every sum (knot_kkt.h): one workgroup per knot;  hv_c = (H v)_c exactly as hipnlp_hess_times_device sums it (+0.0 for the six
 * horizon-global variables),  jt_c = (J^T w)_c exactly as hipnlp_jac_transpose_times_device sums it without a gradient,
 * top_c = hv_c + jt_c,  with dx_dev: top_c = fma(d_x,c, v_c, hv_c + jt_c);  jv_i = (J v)_i exactly as hipnlp_jac_times_device sums it by
 * the row's owner knot,  bottom_i = jv_i,  with dc_dev: bottom_i = fma(-d_c,i, w_i, jv_i).  Without diagonals the result is bit for bit the
 * composition of the three launches and one addition; the same bits at every position of a batch and for both jac orders.  Every element
 * of top_dev and bottom_dev is written exactly once; nothing else is written.
 *
 * Returns HIPNLP_E_INVALID for a missing handle or required pointer (all but dx_dev and dc_dev), HIPNLP_E_UNSUPPORTED on a multi-device
 * handle, on a shard handle (knot_begin / knot_end not the whole horizon) and for a layout whose tables exceed what the kernel stages
 * (hipnlp_last_error says which).  No HIPNLP_E_PARAMS.  Replayable from a captured graph after one eager call on the handle (tests/test_gpu_graph_replay.py). */
int hipnlp_kkt_times_device(hipnlp_handle* h, const double* hess_values_dev, const double* jac_values_dev, const double* dx_dev,
                            const double* dc_dev, const double* v_dev, const double* w_dev, double* top_dev, double* bottom_dev,
                            void* stream);

/* Preconditioned MINRES (Paige and Saunders) on that operator, for every trajectory of the batch at once, resident on the device:
 *
 *     K [sol_top; sol_bottom] = [rhs_top; rhs_bottom],   K = [[H + diag d_x, J^T], [J, -diag d_c]]
 *
 * from the two value runs and the diagonals of hipnlp_kkt_times_device (same rules).  The start is zero (a caller who wants a warm start
 * solves for the correction).  The preconditioner M^-1 = diag(minv_top_dev [batch][n], minv_bottom_dev [batch][m]) > 0 is the caller's;
 * both NULL: the identity, nothing is read.  hipnlp_kkt_diag_precond_device (below) builds a diagonal one.  rhs_top_dev, sol_top_dev [batch][n];
 * rhs_bottom_dev, sol_bottom_dev [batch][m]; iterations_dev, status_dev (int32) and residual_dev [batch].  residual is phibar / beta1:
 * the relative residual in the M^-1 norm, sqrt(r . M^-1 r) / sqrt(b . M^-1 b), as the recurrence estimates it.
 *
 * Status per trajectory: 0 converged, phibar <= rtol beta1 (this includes rhs = 0: zero iterations, sol = 0);  1 the iteration limit;
 * 2 breakdown: r . M^-1 r < 0 or a non-finite alfa, beta or gamma — M is not positive definite or the data is not finite; the trajectory
 * stops with the last finite sol (at the start: sol = 0, residual 1).  Once a trajectory has a final status it is FROZEN: the launches
 * that follow leave its vectors, scalars, sol, iterations, residual and status bit for bit as they are.
 *
 * Launches (knot_minres.h has the recurrence and every expression): two for the start, three per iteration, all on the grid
 * (knots, batch) of the operator.  No workgroup waits for another, no atomics, no persistent kernel: every reduction over a trajectory
 * crosses a launch boundary, and the scalars of the recurrence never visit the host (two records per trajectory, read and written by
 * iteration parity).  Order of every sum: y = K v exactly as hipnlp_kkt_times_device sums it, then y -= (beta/oldb) r1 by one fused
 * multiply-add per element;  a dot product is, per knot, ONE chain of fused multiply-adds per thread from +0.0 over the elements the
 * knot's workgroup of the operator writes (its element of the top, then its first, then its second row), the tree of the grad f . v
 * partial of hipnlp_jac_times_device over the 256 threads, and then the N per-knot partials from +0.0 in ascending knot order, added
 * by every workgroup of the next launch for itself (at every N: there is no reduce launch).  Divisions and square roots are correctly
 * rounded.  So the same bits at every position of a batch, for both jac orders, and for every check_every.
 *
 * check_every == 0: exactly max_iterations iterations are enqueued on `stream` and the call never synchronises (frozen trajectories
 * make the surplus a no-op).  check_every == k > 0: after every k iterations the [batch] statuses are copied into a pinned block of the
 * handle and the stream is waited for; enqueuing stops once no trajectory is still running.  That copy and wait is the only
 * synchronisation, and check_every changes no output bit.  (A call with check_every > 0 cannot be captured into a graph.)
 *
 * The workspace — six vectors of n + m per trajectory (v, y, r1, r2, w, w2; w1 of the recurrence needs no storage), two runs of per-knot
 * partials and the scalar records — belongs to the handle: allocated by hipnlp_kkt_minres_reserve (bytes_out, optional: its size) or by
 * the first solve, freed with the handle.  It is ONE per handle: solves on one handle must be ordered on one stream (or by the
 * caller's events).  The outputs may not alias the inputs; nothing but the six outputs and the workspace is written.
 *
 * NOT claimed: convergence on the KKT systems of real iterates — they are indefinite and badly scaled (entries reach 1e8 on the stairs
 * terrain).  The tests converge on conditioned synthetic value runs, and on symmetrically rescaled ones (cond up to 1e16) with the diagonal
 * of hipnlp_kkt_diag_precond_device; what that diagonal did on real value runs is recorded there.
 *
 * Returns as hipnlp_kkt_times_device (HIPNLP_E_INVALID for a missing handle or required pointer — all but dx_dev, dc_dev and the two
 * minv; HIPNLP_E_UNSUPPORTED on a multi-device handle, a shard handle, a layout beyond the caps), and HIPNLP_E_INVALID for rtol < 0,
 * max_iterations < 0, check_every < 0 and for exactly one of the two minv pointers.
 * With check_every = 0: replayable from a captured graph after one eager call on the handle; every replay starts from zero, whatever
 * status the previous replay or a solve in between left in the workspace (tests/test_gpu_graph_replay.py). */
int hipnlp_kkt_minres_device(hipnlp_handle* h, const double* hess_values_dev, const double* jac_values_dev, const double* dx_dev,
                             const double* dc_dev, const double* minv_top_dev, const double* minv_bottom_dev, const double* rhs_top_dev,
                             const double* rhs_bottom_dev, double* sol_top_dev, double* sol_bottom_dev, double rtol, int max_iterations,
                             int check_every, int32_t* iterations_dev, double* residual_dev, int32_t* status_dev, void* stream);
int hipnlp_kkt_minres_reserve(hipnlp_handle* h, int64_t* bytes_out);

/* The diagonal preconditioner of that solve, built on the device from the same two value runs and diagonals, in ONE launch on the
 * operator's grid (knots, batch):
 *
 *     minv_top_dev    [batch][n]:  1 / max(|H_jj + d_x,j|, floor)      H_jj: the stored diagonal entry of variable j, +0.0 where the pattern
 *                                                                      has none (the six horizon-global variables)
 *     minv_bottom_dev [batch][m]:  1 / max(|d_c,i + sum_e J_ie^2 minv_top_col(e)|, floor)
 *
 * ready to be passed to hipnlp_kkt_minres_device.  The absolute value on the top is deliberate: H + diag d_x is indefinite at real
 * iterates and MINRES needs M positive definite.  dx_dev / dc_dev may be NULL (that term is left out, nothing is read); floor > 0 keeps
 * the reciprocals finite.  A NaN or an infinity in the inputs is not clamped away: every output that depends on it is NaN, and the solve
 * ends that trajectory with status 2.  Pointer, stream and aliasing rules of hipnlp_kkt_times_device.
 *
 * Order of every sum (knot_kkt_precond.h has the rounding sequence): the divisions are correctly rounded; a row's sum is ONE chain from
 * +0.0 over its entries in the order of hipnlp_jac_times_device (ascending global column), per entry q = J_ie * J_ie rounded, then one
 * fused multiply-add with minv_top of the column; d_c,i is added last.  No workgroup waits for another and there are no atomics: the
 * workgroup of a row's owner knot recomputes minv_top of the columns it needs (its own knot's, its predecessor's, the other horizon
 * end's, the globals') from one Hessian value and one d_x each.  So the same bits at every position of a batch and for both jac orders.
 * Every element of minv_top_dev and minv_bottom_dev is written exactly once, by the workgroup that writes that element of
 * hipnlp_kkt_times_device's outputs; nothing else is written.  No workspace.
 *
 * What is claimed: on symmetrically rescaled systems K' = S K S the preconditioned iteration count is, up to rounding, that of the
 * unscaled system (the tests: status 0 after 23 to 25 iterations at cond(K') about 1e12, where the identity ends at status 1 after 300).  On
 * the real N = 4 value runs of the tests (d_x, d_c in U[1, 2]: not an interior-point method's) the diagonal was the difference between
 * status 0 (after about 2 200 iterations) and status 1 at 3 000 on the stairs terrain, and about a fifth fewer iterations on the planar one.
 * NOT claimed: that an interior-point step is cheap with it, or anything about larger systems beyond what profiles/r13_kkt_precond.txt
 * records (at 100 and 200 knots no trajectory converged within 3 000 iterations, with or without it).
 *
 * Returns as hipnlp_kkt_times_device (HIPNLP_E_INVALID for a missing handle or required pointer — all but dx_dev and dc_dev;
 * HIPNLP_E_UNSUPPORTED on a multi-device handle, a shard handle, a layout beyond the caps), and HIPNLP_E_INVALID for a floor that is not
 * a finite number > 0.  Replayable from a captured graph after one eager call on the handle (tests/test_gpu_graph_replay.py). */
int hipnlp_kkt_diag_precond_device(hipnlp_handle* h, const double* hess_values_dev, const double* jac_values_dev, const double* dx_dev,
                                   const double* dc_dev, double floor, double* minv_top_dev, double* minv_bottom_dev, void* stream);

/* A block top for that preconditioner, and the inertia of every knot's block of H + diag d_x (hippopt_amd/csrc/knot_ldl.h):
 *
 *     M^-1 = blockdiag_k( P_k^T L_k^-T |D_k|^-1 L_k^-1 P_k )  (+)  diag(minv_top of the six globals)  (+)  diag(minv_bottom)
 *
 * The Hessian of the Lagrangian is block diagonal by knot (189 variables each; a periodicity coupling of the horizon ends, where the
 * pattern has one, is left out of the blocks), so one workgroup holds a block's packed lower triangle (17 955 doubles) in its LDS and
 * factors it by Bunch-Kaufman partial pivoting, the algorithm and the pinned choices of hipnlp_pose_kkt_ldl_device.  |D| replaces every
 * eigenvalue of D by max(|lambda|, floor): M is symmetric positive definite whatever the inertia of the blocks.  minv_top_dev (read at the
 * six globals only) and minv_bottom_dev are hipnlp_kkt_diag_precond_device's outputs.
 *   hipnlp_kkt_block_bytes           bytes_out[4]: the bytes of factor_dev, pivots_dev, e_dev, o_dev for this handle's batch and horizon
 *                                    (the factor is 143 640 B per knot and trajectory)
 *   hipnlp_kkt_block_factor_device   ONE launch, a workgroup of 1 024 threads per (knot, trajectory): assembles H_k + diag d_x,k (dx_dev
 *                                    may be NULL) from the Hessian run, factors it, and stores per (trajectory, knot): factor_dev
 *                                    [batch][N][17955] (L and D, packed lower triangle by columns, every interchange applied to whole
 *                                    rows of L), pivots_dev [batch][N][189] int32 (bits 0..15 LAPACK's ipiv as int16, bits 16..23 the
 *                                    permutation, bits 24..25: 0 a 1x1 pivot, 1 / 2 the first / second index of a 2x2 block), e_dev and
 *                                    o_dev [batch][N][189] (|D|^-1: its diagonal, and the coupling of index i to i + 1), inertia_dev
 *                                    [batch][N][3] int32 (positive, negative, zero) and status_dev [batch][N] int32: 0 factored; 2 a value
 *                                    that is not finite — that knot's factor, e and o are NaN in every word, its inertia (0, 0, 0).  A
 *                                    pivot column that is exactly zero counts as ONE zero and the factorisation goes on.  Nothing is
 *                                    retried or regularised.  Every word of the six arrays is written.
 *   hipnlp_kkt_block_apply_device    ONE launch: [z_top; z_bottom] = M^-1 [r_top; r_bottom] from the stored arrays; a knot with status
 *                                    2 yields NaN for its 189 elements.  The outputs may not alias the inputs.
 *   hipnlp_kkt_minres_block_device   hipnlp_kkt_minres_device with this M^-1: its arguments plus the four stored arrays; the first
 *                                    launch of every iteration applies the knot's factor in its first wave.  Statuses as there: a knot
 *                                    with status 2 ends its trajectory with status 2.
 * Every element is one fixed chain of fused multiply-adds: the same bits on every launch, at every batch position.  HIPNLP_E_INVALID: a
 * null handle or required pointer (all but dx_dev / dc_dev), a floor that is not a finite number > 0, rtol < 0, max_iterations < 0,
 * check_every < 0 — refused before anything is launched.  HIPNLP_E_UNSUPPORTED as hipnlp_kkt_diag_precond_device.  Measured:
 * profiles/r16_kkt_block.txt (tools/kkt_block_probe.py).  NOT claimed: that an interior-point step is cheap with it; systems with
 * diagonals a factor 1e-4 smaller than U[1, 2] were not seen to converge with either preconditioner.
 * The factor, the apply and (with check_every = 0) the solve: replayable from a captured graph after one eager call on the handle
 * (tests/test_gpu_graph_replay.py). */
int hipnlp_kkt_block_bytes(const hipnlp_handle* h, int64_t* bytes_out /*[4]*/);
int hipnlp_kkt_block_factor_device(hipnlp_handle* h, const double* hess_values_dev, const double* dx_dev /*or NULL*/, double floor, double* factor_dev,
                                   int32_t* pivots_dev, double* e_dev, double* o_dev, int32_t* inertia_dev, int32_t* status_dev, void* stream);
int hipnlp_kkt_block_apply_device(hipnlp_handle* h, const double* factor_dev, const int32_t* pivots_dev, const double* e_dev, const double* o_dev,
                                  const double* minv_top_dev, const double* minv_bottom_dev, const double* r_top_dev, const double* r_bottom_dev, double* z_top_dev,
                                  double* z_bottom_dev, void* stream);
int hipnlp_kkt_minres_block_device(hipnlp_handle* h, const double* hess_values_dev, const double* jac_values_dev, const double* dx_dev /*or NULL*/,
                                   const double* dc_dev /*or NULL*/, const double* factor_dev, const int32_t* pivots_dev, const double* e_dev, const double* o_dev,
                                   const double* minv_top_dev, const double* minv_bottom_dev, const double* rhs_top_dev, const double* rhs_bottom_dev,
                                   double* sol_top_dev, double* sol_bottom_dev, double rtol, int max_iterations, int check_every, int32_t* iterations_dev,
                                   double* residual_dev, int32_t* status_dev, void* stream);

/* The inertia-correcting ladder of that factorisation, climbed by every knot on its own inside ONE launch (knot_ldl.h LADDER): the
 * arguments and the six stored arrays of hipnlp_kkt_block_factor_device, plus delta_init, kappa, max_tries (0 .. 16) and two outputs,
 * delta_dev [batch][N] and tries_dev [batch][N] int32.  Try 0 is hipnlp_kkt_block_factor_device's factorisation (delta = 0).  Try t >= 1
 * assembles the block again from the Hessian run with delta_t added to all 189 diagonal elements — (H_cc + d_x,c) + delta_t, delta_1 =
 * delta_init, delta_(t+1) = delta_t * kappa, one rounded product per try — and factors it again, whole.  A knot leaves the ladder at its
 * first try with the inertia (189, 0, 0), at a try whose data is not finite, or at try max_tries; all eight arrays hold its LAST try.
 * status_dev: 0 the stored factor has the inertia stored beside it, which with max_tries > 0 is (189, 0, 0); 2 a value that is not finite
 * (NaN records as hipnlp_kkt_block_factor_device, inertia (0, 0, 0)); 3 the ladder was exhausted: the factor and the complete inertia of
 * try max_tries are stored, and it is not (189, 0, 0).  There is no status 1: a pivot column that is exactly zero counts as one zero, the
 * factorisation goes on, and the ladder climbs.  max_tries = 0 is one factorisation: the bits of hipnlp_kkt_block_factor_device in all
 * six arrays, status 0 or 2, delta 0, tries 0 (delta_init and kappa are then not read).
 *
 * What status 0 with max_tries > 0 gives: every pivot is 1x1 and positive, so o = 0, e = 1 / d (where no d is below the floor), and
 * hipnlp_kkt_block_apply_device / hipnlp_kkt_minres_block_device apply the INVERSE of H_k + diag d_x,k + delta_k I from this record.
 * With every knot at status 0, d_x > 0 at the six globals and d_c > 0 everywhere, the matrix
 *     K' = [ A   J^T ; J   -diag d_c ],   A = blockdiag_k(H_k + diag d_x,k + delta_k I)  (+)  diag(d_x of the six globals)
 * is symmetric quasi-definite: its inertia is exactly (n, m, 0), the figure IPOPT's regularisation loop is driven by, and nobody had to
 * factor K'.  (K' is the operator with d_x' = d_x + delta_k on knot k's variables; a periodicity coupling of the horizon ends that the
 * Hessian pattern has lies outside every block and is NOT covered by this statement.)  The limit: this is a SUFFICIENT correction and a
 * conservative one, NOT IPOPT's criterion.  IPOPT needs only the Hessian reduced to the null space of J positive definite and adds one
 * delta to the whole top block; a delta per knot that makes every whole block positive definite can be larger than that needs.
 * delta_init and kappa have no defaults here; nothing about MINRES's convergence on K' is claimed.  Cost: (tries + 1) whole
 * factorisations for the slowest knot of a launch; measured: profiles/r17_kkt_ladder.txt (tools/kkt_ladder_probe.py).
 * HIPNLP_E_INVALID, refused before anything is launched: what hipnlp_kkt_block_factor_device refuses, a null delta_dev or tries_dev,
 * max_tries outside 0 .. 16, and with max_tries > 0 a delta_init that is not a finite number > 0 or a kappa that is not a finite number
 * > 1.  HIPNLP_E_UNSUPPORTED as hipnlp_kkt_block_factor_device.  Replayable from a captured graph after one eager call on the handle (tests/test_gpu_graph_replay.py). */
int hipnlp_kkt_block_ladder_device(hipnlp_handle* h, const double* hess_values_dev, const double* dx_dev /*or NULL*/, double floor, double delta_init, double kappa,
                                   int max_tries, double* factor_dev, int32_t* pivots_dev, double* e_dev, double* o_dev, int32_t* inertia_dev, int32_t* status_dev,
                                   double* delta_dev /*[batch][N]*/, int32_t* tries_dev /*[batch][N]*/, void* stream);

/* The CONDENSED block factorisation (knot_condense.h), ONE launch on hipnlp_kkt_block_factor_device's mapping: where d_c > 0 the bottom
 * block of K is eliminated instead of approximated,
 *     C = H + diag d_x + J^T diag(1 / d_c) J,      In(K) = (0, m, 0) + In(C)   (Haynsworth),
 * and every knot factors the diagonal block of C it can form alone, B_k = H_k + diag d_x,k + J_k^T diag(1 / d_c) J_k, J_k the knot's
 * column block of the stored jac run.  The six stored arrays have hipnlp_kkt_block_factor_device's format and status convention, so
 * hipnlp_kkt_block_apply_device and hipnlp_kkt_minres_block_device take them as they are.  Assembly: that factorisation's, then per
 * element (r, c) one acc = fma(a_ir, a_ic * s_i, acc), s_i = 1 / d_c,i correctly rounded, for every row i of g with an entry in both
 * columns, in ascending global row: one writer and one chain per element, no atomics, the same bits in every launch, at every batch
 * position and in both orders of jac g.
 * The launch also writes ALL of minv_top_dev [batch][n] and minv_bottom_dev [batch][m] — a condensed DIAGONAL preconditioner on their own
 * (hipnlp_kkt_minres_device) and what the block apply reads for the six globals and the bottom:
 *     minv_bottom_i = 1 / d_c,i;   minv_top_j = 1 / max(|B_k,jj|, floor);   six globals: 1 / max(|d_x,g + sum_i J_ig^2 / d_c,i|, floor).
 * status_dev: 0 factored; 2 the knot's block data is not finite, OR a d_c,i of a row of g touching the knot's column block is not a
 * finite number > 0: NaN in every word of its factor, e and o, inertia (0, 0, 0); minv_bottom_i of such a row is NaN.
 * What inertia_dev proves: every B_k is a principal submatrix of C, so a B_k with a negative or zero eigenvalue proves that K does NOT
 * have the inertia (n, m, 0).  All B_k positive definite proves nothing about K: the off-diagonal blocks of C are not looked at.  Nothing
 * is retried or regularised; a periodicity coupling of the Hessian pattern stays outside every block.
 * HIPNLP_E_INVALID, refused before anything is launched: a null dc_dev or jac_values_dev, and what hipnlp_kkt_block_factor_device refuses,
 * a null minv_top_dev or minv_bottom_dev.  HIPNLP_E_UNSUPPORTED as hipnlp_kkt_block_factor_device (multi-device and shard handles
 * included), and a layout whose column block has more than 1 620 entries or is touched by more than 439 rows.
 * Measured: 1.14 x hipnlp_kkt_block_factor_device's launch at 100 x 1, 100 x 64 and stairs 200 x 16 (profiles/r18_kkt_condensed.txt,
 * tools/kkt_condensed_probe.py).  Replayable from a captured graph after one eager call on the handle (tests/test_gpu_graph_replay.py). */
int hipnlp_kkt_condensed_factor_device(hipnlp_handle* h, const double* hess_values_dev, const double* jac_values_dev, const double* dx_dev /*or NULL*/,
                                       const double* dc_dev /*required*/, double floor, double* factor_dev, int32_t* pivots_dev, double* e_dev, double* o_dev,
                                       int32_t* inertia_dev, int32_t* status_dev, double* minv_top_dev /*[batch][n]*/, double* minv_bottom_dev /*[batch][m]*/, void* stream);

/* Sharded variant (multi-GPU): the handle owns knots [knot_begin, knot_end).  Outputs are
 * shard-local and contiguous so that one RCCL all-gather reassembles them:
 *   grad_shard [batch][shard_grad]  = grad f entries of the shard's knots (+ the 6 global entries on the last shard)
 *   jac_shard  [batch][shard_nnz]   = the CCS value run of the shard's column blocks
 *   g_stage    [batch][nk][HIPNLP_G_STAGE] knot-major staging of the rows each knot owns; hipnlp_stage_rows()
 *              gives the global row of every staging slot (-1 = unused) for the scatter after the gather
 *   f_dev      [batch] partial cost of the shard's knots                                                     */
#define HIPNLP_G_STAGE 550
int hipnlp_eval_device_shard(hipnlp_handle* h, const double* x_dev, double* f_dev, double* grad_shard,
                             double* g_stage, double* jac_shard, void* stream);
int hipnlp_stage_rows(const hipnlp_handle* h, int k, int32_t* rows /*[HIPNLP_G_STAGE]*/);
/* Reassembly behind the all-gather of the fused shard buffers: out[i] = gathered[src[i]] (i < count: [grad | jac | g] in reference
 * order) and *f_out = sum over ranks, in rank order, of gathered[r * shard_len] (the cost partials); device pointers on the current
 * device, enqueued on `stream`, not synchronised.  Stateless (no handle): `stream` must be the stream the shard evaluation and the
 * all-gather were enqueued on (a NULL stream here is the legacy default stream, which nothing orders against a handle's own
 * stream: hippopt_amd/sharded.py passes one explicit stream to both calls). */
int hipnlp_reassemble(const double* gathered_dev, const int64_t* src_dev, double* out_dev, int64_t count, int world, int64_t shard_len,
                      double* f_out_dev, void* stream);

/* ---- the same exchange WITHOUT a collective: peer stores over xGMI (one process per GPU) ----------------------------
 * xGMI is point to point: instead of a ring all-gather followed by a reassembly pass, every rank pushes its fused shard buffer —
 * entry by entry, already at its position in the reference's order — into the output buffer of EVERY rank (its own included) with
 * one kernel of plain stores, then raises its flag in every rank's flag array; a rank's outputs are complete when all `world` flags
 * carry the step number.  The buffers live in fine-grained device memory shared through HIP IPC handles (64 bytes each, moved
 * between the processes by any channel: hippopt_amd/sharded.py uses torch.distributed's object gather once, at set-up); nothing here
 * depends on torch or RCCL.  All calls are enqueued on `stream` of the CURRENT device and not synchronised.
 *   hipnlp_ipc_alloc   fine-grained (uncached) device memory on `device`, zeroed, + its IPC handle
 *   hipnlp_ipc_open    maps a peer's allocation into this process (enables peer access to its device on demand)
 *   hipnlp_peer_push   peer_out[r][dst[i]] = shard[i] for every rank r and every i < count with dst[i] >= 0 (peer_out: a DEVICE array
 *                      of `world` device pointers)
 *   hipnlp_peer_signal system-scope fence, then peer_flags[r][rank] = seq for every r < world (peer_flags: device array of `world` pointers —
 *                      every rank's flag array, or a subset: gather_to_root signals rank 0 alone; rank < 64: this rank's slot)
 *   hipnlp_peer_signal_checked  the same, but with bit 63 set in the value when *status_dev != 0 at that point of the stream: the step of
 *                      THIS rank has failed (a wait of its own gave up), what it pushed must not pass for an evaluation on the
 *                      receiving side either — hipnlp_peer_wait takes a flag with that bit for "arrived, poisoned" (seq < 2^63)
 *   hipnlp_peer_wait   spins (bounded: ~2^20 polls — about a second) until flags[r] >= seq for all r, then
 *                      out[f_off + world] = sum over r, in rank order, of out[f_off + r] (the cost partials).  A wait that gives up
 *                      is sticky and loud: *status_dev is OR-ed with 1 (never cleared here: the host zeroes it when it sets the
 *                      exchange up) and the whole step is poisoned — out[0 .. f_off) and the cost become NaN — so that pushes that
 *                      may be partial cannot pass for an evaluation; a flag that carries the poison bit does the same              */
#define HIPNLP_IPC_HANDLE_BYTES 64
int hipnlp_ipc_alloc(size_t bytes, int device, void** dev_ptr, void* handle_out /*[HIPNLP_IPC_HANDLE_BYTES]*/);
int hipnlp_ipc_open(const void* handle /*[HIPNLP_IPC_HANDLE_BYTES]*/, int device, void** dev_ptr);
int hipnlp_ipc_close(void* dev_ptr);
int hipnlp_ipc_free(void* dev_ptr);
int hipnlp_peer_push(const double* shard_dev, const int64_t* dst_dev, int64_t count, double* const* peer_out_dev, int world, void* stream);
int hipnlp_peer_signal(unsigned long long* const* peer_flags_dev, int world, int rank, unsigned long long seq, void* stream);
int hipnlp_peer_signal_checked(unsigned long long* const* peer_flags_dev, int world, int rank, unsigned long long seq, const int* status_dev,
                               void* stream);
int hipnlp_peer_wait(const unsigned long long* flags_dev, int world, unsigned long long seq, double* out_dev, int64_t f_off,
                     int* status_dev, void* stream);
/* The push folded into the evaluation: the knot kernel of a shard handle (batch 1, at most 256 knots in the shard) stores the shard's
 * grad f / jac g / g entries — at their FINAL positions — and the shard's cost straight into the buffer of every rank,
 *     peer_out[r] = [grad f (n) | jac g (nnz) | g (m) | cost partial of rank 0 .. world-1 | f]      (n, m, nnz of the whole problem),
 * the layout hipnlp_peer_push fills (f_off = n + nnz + m for hipnlp_peer_wait): the transfers over the links overlap with the knot
 * programs still running, and neither a push nor a reassembly launch follows.  peer_out_dev: DEVICE array of `world` device-visible
 * base addresses (hipnlp_ipc_alloc / hipnlp_ipc_open) — the buffers this call stores into: every rank's, or rank 0's alone
 * (world = 1: gather_to_root, one consumer); rank: the slot of this shard's cost partial (< 64; the buffers hold one slot per rank
 * of the job, whatever `world` is here).  Then hipnlp_peer_signal and hipnlp_peer_wait as above.  Enqueued on `stream`
 * (NULL: the handle's own stream), not synchronised; the non-finite flag of the handle works as with hipnlp_eval_device. */
int hipnlp_eval_device_peers(hipnlp_handle* h, const double* x_dev, double* const* peer_out_dev, int world, int rank, void* stream);

/* ---- Exchanges without the constants of jac g (multi-GPU) ---------------------------------------------------------------
 * 43 % of the Jacobian pattern of the kinodynamic NLP never changes between callbacks: the +-1 / -dt/2 / mass entries of the linear rows the
 * transcription emits (trapezoid defects and x_0 rows: /root/reference/src/hippopt/base/multiple_shooting_solver.py:713-742,
 * integrators/implicit_trapezoid.py:24-39).  An exchange between GPUs — the bound of the knot-sharded path — has no reason to move
 * them every step: on a handle created with HIPNLP_FLAG_JAC_VARYING_FIRST the shards hand over the VARYING RUN of every knot block
 * only, and the consumer's buffer (the reassembled array on every rank, rank 0's gather buffer, a shared host sink) holds the constant
 * entries, put there once per parameter set by hipnlp_fill_jac_constants.  All of these need HIPNLP_FLAG_JAC_VARYING_FIRST
 * (HIPNLP_E_UNSUPPORTED otherwise) and hipnlp_set_params first; device pointers, enqueued on `stream` (NULL: the handle's own), not
 * synchronised.
 *   hipnlp_jac_vary_layout         out[0..2] varying entries of a first / interior / last knot block, out[3] of the whole horizon,
 *                                  out[4] of the knots in front of this handle's first knot, out[5] of this handle's knots: a COMPACT
 *                                  destination lists the varying runs of the knot blocks behind one another (knot k's run at
 *                                  out[0] + (k - 1) out[1] for k >= 1), entry i of a run being entry i of the knot's block in the pattern
 *                                  (hipnlp_sparsity; hipnlp_jac_constant_mask is 0 exactly there)
 *   hipnlp_fill_jac_constants      the constant entries (values under the parameters last set) into jac_dev [batch][nnz], a complete
 *                                  value array in the handle's pattern order: of the handle's own knots, or — whole_horizon != 0 — of every
 *                                  knot and the horizon-global columns (a shard handle knows the whole pattern: the reassembled buffer
 *                                  of a rank is filled by that rank).  Again after every hipnlp_set_params that changes dt or the mass.
 *   hipnlp_eval_device_vary        hipnlp_eval_device with a compact jac destination: jac_vary_dev [batch][out[3]]
 *   hipnlp_eval_device_shard_vary  hipnlp_eval_device_shard with a compact jac shard: jac_vary_shard [batch][out[5]] — and a compact
 *                                  staging of g: g_stage [batch][shard_g_rows] lists, knot behind knot, the rows each knot owns in the
 *                                  order of its staging slots (the entries >= 0 of hipnlp_stage_rows(k), in slot order), instead of
 *                                  HIPNLP_G_STAGE slots per knot of which half are unused
 *   hipnlp_eval_device_peers_vary  hipnlp_eval_device_peers storing the varying runs only, at their places in the pattern, into buffers
 *                                  whose jac part holds the constants (hipnlp_fill_jac_constants(..., whole_horizon = 1) on the buffer's
 *                                  owner)
 *   hipnlp_reassemble_scatter      hipnlp_reassemble with a destination index: out[dst[i]] = gathered[src[i]], i < count — entries of
 *                                  `out` no shard sends (the constants) are left alone                                                 */
int hipnlp_jac_vary_layout(const hipnlp_handle* h, int64_t* out /*[6]*/);
int hipnlp_fill_jac_constants(hipnlp_handle* h, double* jac_dev, int whole_horizon, void* stream);
int hipnlp_eval_device_vary(hipnlp_handle* h, const double* x_dev, double* f_dev, double* grad_dev, double* g_dev, double* jac_vary_dev, void* stream);
int hipnlp_eval_device_shard_vary(hipnlp_handle* h, const double* x_dev, double* f_dev, double* grad_shard, double* g_stage, double* jac_vary_shard,
                                  void* stream);
int hipnlp_eval_device_peers_vary(hipnlp_handle* h, const double* x_dev, double* const* peer_out_dev, int world, int rank, void* stream);
int hipnlp_reassemble_scatter(const double* gathered_dev, const int64_t* src_dev, const int64_t* dst_dev, double* out_dev, int64_t count, int world,
                              int64_t shard_len, double* f_out_dev, void* stream);

/* ---- One caller, several devices ---------------------------------------------------------------------------------------------------------
 * The reference has ONE caller of the callbacks: IPOPT, in the process that runs self._solver.solve()
 * (/root/reference/src/hippopt/base/opti_solver.py:479); x lives in that process's memory and f, grad f, g, jac g are wanted in arrays of
 * its own.  hipnlp_multi_create serves that caller from SEVERAL devices behind the host-buffer entry points above: the handle it returns
 * is used exactly like one of hipnlp_create — hipnlp_set_params, hipnlp_bounds, hipnlp_sparsity, hipnlp_eval, hipnlp_eval_pinned,
 * hipnlp_eval_hess / _at, hipnlp_hess_nnz / _sparsity, hipnlp_cost_terms, the hipnlp_set_* switches of the host path, hipnlp_host_stats,
 * the hipnlp_ipopt_* callbacks, hipnlp_destroy — with the same results:
 *   - the horizon is cut into n_devices contiguous knot ranges, the first (horizon mod n_devices) of them one knot longer; the rows of the
 *     trapezoid defect of interval k -> k + 1 belong to the owner of knot k + 1 (the naming of base/multiple_shooting_solver.py:713-742),
 *     so a shard READS the record of the knot in front of its first one (the halo) besides its own, the six horizon-global variables, and
 *     the record of the other horizon end where it owns knot 0 or knot N - 1 (periodicity rows); one shard handle per entry of devices[]
 *     (a device may be named more than once: its shards then share it — how the path is tested on one card);
 *   - an evaluation copies x ONCE into a pinned block that the kernels of every device read over their own link (big batches: each shard
 *     copies the records it reads into its own HBM first, on its own stream), launches every shard's kernel — which stores the shard's
 *     entries of grad f, g and jac g AT THEIR FINAL PLACES in the caller's arrays (registered: hipnlp_host_register, or by the handle at
 *     their second sight) or in the handle's pinned block, over that device's own link — and waits for all of them.  No data moves
 *     between the devices and nothing is reassembled;
 *   - f and the per-term costs are summed by the caller's thread from the knots' partials (96 B per knot, stored to pinned memory by the
 *     knot workgroups) in the order of the device reduction: bit for bit the f of one handle over the whole horizon, whatever the cut;
 *     grad f, g, jac g and the Hessian values are those of the knot programs, which do not depend on the cut either (a shard small
 *     enough to be resident at once runs the eight-wave instantiation of the same program, hipnlp_multi_info: equal to 1e-13, not bit
 *     for bit, where that differs from the instantiation one handle over the whole horizon would run);
 *   - an output that is NOT brought to the host by its evaluation (hipnlp_set_prefetch) stays in the shards' HBM; grad f and jac g are
 *     fetched from there when a later new_x = 0 call asks (one copy per shard), g — scattered over the constraint blocks — is evaluated again.
 * The device-resident entry points (hipnlp_eval_device*, hipnlp_eval_hess_device, hipnlp_fill_jac_constants, the profiling calls) answer
 * HIPNLP_E_UNSUPPORTED on such a handle: they belong to one device.
 *   hipnlp_multi_create     desc: the whole horizon (knot_begin = knot_end = 0; desc->device is ignored); devices[n_devices]: HIP ordinals
 *   hipnlp_multi_info       *n_shards: in = capacity of the arrays, out = shards of the handle (0: a plain handle); devices / knot_begin /
 *                           knot_end / waves (4 or 8: the instantiation of the knot kernel the shard launches) may be NULL
 *   hipnlp_multi_breakdown  us[n_shards][2]: host clock of the last evaluation from the start of the launch loop — shard i enqueued,
 *                           shard i seen complete (the shards are waited for in order).  Diagnostic.
 * MEASURED on one card only (several shards of one device, tests/test_gpu_multi.py, bench.py `one_caller`); with one device per shard:
 * unmeasured in this repository. */
int hipnlp_multi_create(const hipnlp_desc* desc, const int32_t* devices, int n_devices, hipnlp_handle** out);
/* The cut and what of x a shard reads — pure arithmetic, no device (what hipnlp_multi_create follows): knots [*knot_begin, *knot_end) of
 * shard `shard` of n_shards, and x_ranges[4][2] = {offset, count} in doubles of one trajectory's x: [0] the shard's records with the halo
 * record in front of them, [1] the six horizon-global variables, [2] the last knot's record for the owner of knot 0, [3] the first knot's
 * record for the owner of the last knot (count 0: not read).  A shard's kernel reads x NOWHERE else: a caller that keeps x in pieces
 * (or a transport that ships it) needs to deliver exactly these. */
int hipnlp_multi_plan(int horizon, int n_shards, int shard, int32_t* knot_begin, int32_t* knot_end, int64_t* x_ranges /*[4][2]*/);
int hipnlp_multi_info(const hipnlp_handle* h, int32_t* n_shards, int32_t* devices, int32_t* knot_begin, int32_t* knot_end, int32_t* waves);
int hipnlp_multi_breakdown(const hipnlp_handle* h, double* us);
/* One launching thread per shard.  Enqueueing a kernel costs the host 4 - 6 us and waiting for its stream a few more: from the caller's
 * thread, one shard after the other, shard i starts ~i x 10 us behind shard 0 — with eight shards longer than the callback of ONE device.
 * on = 1: shards 1 .. n-1 get a worker thread bound to their device; an evaluation publishes its job, the caller's thread does shard 0's
 * part and waits for the workers.  A worker polls for the next job for spin_us microseconds after its last one (IPOPT's callbacks come in
 * bursts, microseconds apart: default 200; < 0: leave as it is) and then sleeps until woken (IPOPT factorises for milliseconds between
 * bursts: no core is burnt meanwhile, the first callback of a burst pays one wake-up).  on = 0: the caller's thread launches every shard,
 * then waits for every shard.  hipnlp_multi_create turns the threads ON for handles of more than one shard.  Values are the same either way. */
int hipnlp_multi_set_threads(hipnlp_handle* h, int on, double spin_us);

/* Per-named-cost values of the last evaluation (Output.cost_values, base/problem.py:28-56):
 * values[batch][HIPNLP_NCOST_TERMS], summed over knots, in the order of hipnlp_cost_term_name(). */
#define HIPNLP_NCOST_TERMS 12
int hipnlp_cost_terms(hipnlp_handle* h, double* values);
const char* hipnlp_cost_term_name(int i);

/* Row-block directory: name (reference constraint base name), first row, rows per knot, first knot, knots — in the numbering of the
 * FULL subject_to list (m_full rows), whether or not the handle was created with DETECT_SIMPLE_BOUNDS. */
int hipnlp_num_row_blocks(const hipnlp_handle* h);
int hipnlp_row_block(const hipnlp_handle* h, int i, const char** name,
                     int32_t* first_row, int32_t* rows_per_knot, int32_t* first_knot, int32_t* n_knots);

/* Kernel time (ms) of the last TIMED evaluation, measured with hipEvents on the stream the kernels ran on; blocks until
 * that launch has finished.  hipnlp_eval() launches are always timed; hipnlp_eval_device*() launches only when selected by an
 * armed profile (an event record drains the stream and costs microseconds: it must not sit around every device-path launch). */
int hipnlp_last_kernel_ms(hipnlp_handle* h, float* ms);

/* HIP-event timing over a region of launches (bench.py roofline leg).  profile_begin arms up to max_launches event triples;
 * every stride-th launch from then on is bracketed (before the knot kernel, after it, after the reduction kernel) on the
 * launch stream.  profile_end synchronises and returns the mean durations (ms) and the number of timed launches.   */
int hipnlp_profile_begin(hipnlp_handle* h, int max_launches, int stride);
int hipnlp_profile_end(hipnlp_handle* h, double* mean_knot_kernel_ms, double* mean_launch_ms, int* count);
/* Runs instead of single launches: one event before the first and one after the last of every run_len consecutive launches (nothing
 * in between); profile_end then returns the mean duration per launch of the runs (dispatch gaps between the launches of a run
 * included) and the number of launches measured.  For launches so short that an event pair around each would dominate. */
int hipnlp_profile_begin_runs(hipnlp_handle* h, int max_runs, int run_len);
/* Kernel launches behind one device-path evaluation: 1 (trajectories of at most 256 knots in launches of at most 32768 knots: the
 * cost is summed inside the knot launch by one reducer workgroup per trajectory) or 2 (otherwise: knot kernel + cost reduction
 * kernel). */
int hipnlp_kernels_per_eval(const hipnlp_handle* h);

/* =====================================================================================================================
 * Static pose finder (BASELINE config 2): the single-knot NLP of
 *   src/hippopt/turnkey_planners/humanoid_pose_finder/planner.py:323-399 (Planner.__init__) with
 *   _add_contact_point_feasibility :670-722, _add_contact_kinematic_consistency :631-668,
 *   _add_kinematics_constraints :446-519, _add_kinematics_regularization :521-629, _add_foot_regularization :724-768.
 * One handle evaluates `batch` independent poses per launch (one workgroup per pose).
 *
 *   x [81]   reference creation order: per contact point c (left[0..3], right[0..3]): p (3), f (3); base position (3),
 *            base quaternion xyzw (4), joint positions (23), com (3)
 *   p [202]  reference creation order: descriptors 8x3 | mass | parametric_link_length_multipliers (1) |
 *            parametric_link_densities (1) | gravity 6 | references.state: per point p,f,descriptor (9 each) |
 *            base position 3 | base quaternion 4 | joints 23 | com 3 | references.frame_quaternion_xyzw 4 |
 *            left_hand_position 3 | right_hand_position 3 | relaxed_complementarity_epsilon | static_friction |
 *            maximum_joint_positions 23 | minimum_joint_positions 23 | left/right_hand_position_in_frame 3+3
 *   g        subject_to call order: per point {complementarity, height, normal, friction, kinematics_consistency(3)},
 *            unitary_quaternion, com_kinematics_consistency(3), centroidal_momentum_dynamics(6),
 *            joint_position_bounds(23), then the optional sumsqr(.) == 0 rows of com / point positions in subject_to mode
 *            ... and of the left / right hand position (three rows each) in subject_to mode
 *   f        base_quaternion_error, frame_rotation_error, com_position_error, joint_positions_error, per foot the
 *            force average / point position / force regularisations, left / right hand position error (minimize mode)
 * Not built (HIPNLP_E_INVALID): the parametric-link model (adam.parametric; parametric_link_names is None in
 * humanoid_pose_finder/main.py).
 * ===================================================================================================================== */
#define HIPNLP_POSE_NX 81
#define HIPNLP_POSE_NP 202
#define HIPNLP_POSE_NCOST_TERMS 9

typedef struct hipnlp_pose_settings {
    int32_t terrain;                    /* settings.terrain: HIPNLP_TERRAIN_*                       (planner.py:80) */
    int32_t n_terrain_steps;
    hipnlp_terrain_step terrain_steps[HIPNLP_MAX_TERRAIN_STEPS];
    int32_t com_position_type;          /* settings.com_position_expression_type          (planner.py:566-573) */
    int32_t left_point_position_type;   /* settings.left_point_position_expression_type   (planner.py:385-390) */
    int32_t right_point_position_type;  /* settings.right_point_position_expression_type  (planner.py:391-396) */
    int32_t reserved_;
    double base_quaternion_cost_multiplier;
    double desired_frame_quaternion_cost_multiplier;
    double com_regularization_cost_multiplier;
    double joint_regularization_cost_weights[HIPNLP_NJ];
    double joint_regularization_cost_multiplier;
    double force_regularization_cost_multiplier;
    double average_force_regularization_cost_multiplier;
    double point_position_regularization_cost_multiplier;
    /* hand position expressions (planner.py:596-660; a zeroed tail = the settings' default: both skipped):
     *   position of the point hand_position_in_frame (parameter p[196..201]) of the frame settings.left/right_hand_frame_name
     *   == references.left/right_hand_position (p[142..147]);  subject_to: three rows "left_hand_position_error" /
     *   "right_hand_position_error" behind the rows above, in Opti's canonical form of `expression == parameter`: g = the position,
     *   lbg = ubg = the reference;  minimize: multiplier * sumsqr(position - reference)  (base/problem.py:95-174).
     *   The frame is given as in hipnlp_robot_model: the link it is rigidly attached to and link_T_frame. */
    int32_t hand_type[2];               /* settings.left/right_hand_expression_type: HIPNLP_EXPR_*  (planner.py:88, 91) */
    int32_t hand_frame_link[2];
    double hand_frame_R[2][9];
    double hand_frame_o[2][3];
    double hand_regularization_cost_multiplier[2];   /* settings.left/right_hand_regularization_cost_multiplier */
} hipnlp_pose_settings;

typedef struct hipnlp_pose_desc {
    hipnlp_pose_settings settings;
    hipnlp_robot_model model;
    int32_t batch;    /* independent poses per call (>= 1) */
    int32_t device;
    int32_t abi_version;   /* HIPNLP_ABI_VERSION (checked by hipnlp_pose_create) */
    int32_t flags;         /* none defined: 0 */
} hipnlp_pose_desc;

typedef struct hipnlp_pose_dims { int32_t n, m, nnz, np; } hipnlp_pose_dims;
typedef struct hipnlp_pose_handle hipnlp_pose_handle;

/* Same contracts as the hipnlp_* functions of the same name above (shapes with n = 81, np = 202). */
int hipnlp_pose_create(const hipnlp_pose_desc* desc, hipnlp_pose_handle** out);
void hipnlp_pose_destroy(hipnlp_pose_handle* h);
const char* hipnlp_pose_last_error(const hipnlp_pose_handle* h);
int hipnlp_pose_get_dims(const hipnlp_pose_handle* h, hipnlp_pose_dims* out);
int hipnlp_pose_set_params(hipnlp_pose_handle* h, const double* p /*[batch][202]*/);
int hipnlp_pose_bounds(const hipnlp_pose_handle* h, double* lbg, double* ubg /*[batch][m]: bounds of every pose*/);
int hipnlp_pose_sparsity(const hipnlp_pose_handle* h, int32_t* irow, int32_t* jcol);
int hipnlp_pose_eval(hipnlp_pose_handle* h, const double* x, double* f, double* grad_f, double* g, double* jac);
int hipnlp_pose_eval_device(hipnlp_pose_handle* h, const double* x_dev, double* f_dev, double* grad_dev, double* g_dev,
                            double* jac_dev, void* stream);
/* Exact Hessian of the Lagrangian  obj_factor * f(x) + lambda^T g(x)  (IPOPT eval_h: bool eval_h(n, x, new_x, obj_factor, m,
 * lambda, new_lambda, nele_hess, iRow, jCol, values, ud)).  The reference reaches it through CasADi's nlp_hess_l: the pose finder
 * runs IPOPT with its default exact-Hessian option (humanoid_pose_finder/main.py:101 `casadi_solver_options = {}`,
 * planner.py:334-339 -> base/opti_solver.py:123-125,479).  Lower triangle (irow >= jcol), column major, fixed pattern:
 *   hipnlp_pose_hess_nnz / _sparsity   structure (the `values == NULL` call of eval_h)
 *   hipnlp_pose_eval_hess              host buffers: x [batch][81], obj_factor [batch], lambda [batch][m] -> hess [batch][nnz_h]
 *   hipnlp_pose_eval_hess_device       device pointers, enqueued on `stream`, not synchronised                                  */
int hipnlp_pose_hess_nnz(const hipnlp_pose_handle* h, int32_t* nnz_h);
int hipnlp_pose_hess_sparsity(const hipnlp_pose_handle* h, int32_t* irow, int32_t* jcol);
int hipnlp_pose_eval_hess(hipnlp_pose_handle* h, const double* x, const double* obj_factor, const double* lambda, double* hess);
int hipnlp_pose_eval_hess_device(hipnlp_pose_handle* h, const double* x_dev, const double* obj_factor_dev, const double* lambda_dev,
                                 double* hess_dev, void* stream);
/* Products of one pose's derivatives, summed inside the pose's own workgroup from what its program holds in LDS: one kernel launch
 * each, device pointers only, enqueued on `stream` (NULL: the handle's own stream), not synchronised, no host copy.  Neither jac g
 * nor the Hessian is written to memory; the order of every sum is fixed (the same bits on every launch).
 *   hipnlp_pose_eval_lagrangian_grad_device   out [batch][81] = obj_factor grad f(x) + J(x)^T lambda
 *   hipnlp_pose_eval_jac_vec_device           gradf_dot_v [batch] = grad f(x) . v,  jac_v [batch][m] = J(x) v;  either may be NULL, not both
 *   hipnlp_pose_eval_hess_vec_device          out [batch][81] = H(x, obj_factor, lambda) v,  H as hipnlp_pose_eval_hess_device
 * x_dev, v_dev [batch][81], obj_factor_dev [batch], lambda_dev [batch][m].  HIPNLP_E_INVALID: a null handle or required pointer;
 * HIPNLP_E_PARAMS: hipnlp_pose_set_params has not been called.  A non-finite result raises the pose's flag as in the calls above.  */
int hipnlp_pose_eval_lagrangian_grad_device(hipnlp_pose_handle* h, const double* x_dev, const double* obj_factor_dev /*[batch]*/,
                                            const double* lambda_dev /*[batch][m]*/, double* out_dev /*[batch][81]*/, void* stream);
int hipnlp_pose_eval_jac_vec_device(hipnlp_pose_handle* h, const double* x_dev, const double* v_dev /*[batch][81]*/,
                                    double* gradf_dot_v_dev /*[batch] or NULL*/, double* jac_v_dev /*[batch][m] or NULL*/, void* stream);
int hipnlp_pose_eval_hess_vec_device(hipnlp_pose_handle* h, const double* x_dev, const double* obj_factor_dev, const double* lambda_dev,
                                     const double* v_dev, double* out_dev /*[batch][81]*/, void* stream);
/* The KKT chain of a pose from STORED value runs — hess_values_dev [batch][nnz_h] as hipnlp_pose_eval_hess_device and jac_values_dev
 * [batch][nnz] as hipnlp_pose_eval_device of THIS handle wrote them; no pose program runs.
 *
 *     K = [ H + diag d_x    J^T       ]      dx_dev [batch][81], dc_dev [batch][m]: optional (NULL: that term is left out)
 *         [ J              -diag d_c  ]
 *
 * A pose is one workgroup: both runs, the tables and a vector fit in its LDS, every reduction is a tree over the workgroup.  Each call
 * is ONE launch on a grid of `batch` workgroups, enqueued on `stream` (NULL: the handle's own stream), not synchronised; there is no
 * workspace, no reserve call and no check_every, and calls on different streams are independent.  The order of every sum is fixed
 * (hippopt_amd/csrc/pose_kkt.h): the same bits on every launch, at every batch position.  Outputs may not alias inputs.
 *   hipnlp_pose_kkt_times_device         top [batch][81] = (H + diag d_x) v + J^T w,  bottom [batch][m] = J v - diag(d_c) w
 *                                        (hipnlp_kkt_times_device's combinations: top = hv + jt, with d_x one fused multiply-add on top)
 *   hipnlp_pose_kkt_diag_precond_device  minv_top = 1 / max(|H_cc + d_x,c|, floor) (H_cc = 0 where the pattern has no diagonal entry),
 *                                        minv_bottom = 1 / max(|d_c,i + sum_e J_ie^2 minv_top_col(e)|, floor): the arithmetic of
 *                                        hipnlp_kkt_diag_precond_device; a NaN or an infinity of the inputs comes out as NaN
 *   hipnlp_pose_kkt_minres_device        K [sol_top; sol_bottom] = [rhs_top; rhs_bottom] by preconditioned MINRES from a zero start, the
 *                                        recurrence of hipnlp_kkt_minres_device, ALL iterations in the one launch.  M^-1 = diag(minv_top,
 *                                        minv_bottom) > 0 (both NULL: the identity); build_diagonal != 0 (then both NULL) builds the
 *                                        diagonal above inside the same launch — bit for bit the solution of calling
 *                                        hipnlp_pose_kkt_diag_precond_device first and passing its output.  iterations_dev, status_dev
 *                                        [batch] int32, residual_dev [batch] (phibar / beta1, the relative residual in the M^-1 norm).
 *                                        status 0: residual <= rtol; 1: max_iterations reached; 2: breakdown (M not positive definite or
 *                                        data that is not finite; the solution is the last one before it).
 * HIPNLP_E_INVALID: a null handle or required pointer, floor not a finite number > 0, rtol < 0 or NaN, max_iterations < 0 or above
 * 4096 (what one launch may run on a shared device), one of minv_top_dev / minv_bottom_dev alone, or either with build_diagonal.
 * HIPNLP_E_UNSUPPORTED: the handle's pattern is beyond what a workgroup stages (1024 entries of jac g, 256 rows, 768 entries and 1536
 * touches of the Hessian); nothing is truncated.  Measured: hippopt_amd/autograd.py PoseKKTValues.solve and profiles/r14_pose_kkt.txt.
 * All three: replayable from a captured graph after one eager call on the handle (tests/test_gpu_graph_replay.py). */
int hipnlp_pose_kkt_times_device(hipnlp_pose_handle* h, const double* hess_values_dev, const double* jac_values_dev, const double* v_dev /*[batch][81]*/,
                                 const double* w_dev /*[batch][m]*/, double* top_dev /*[batch][81]*/, double* bottom_dev /*[batch][m]*/,
                                 const double* dx_dev /*or NULL*/, const double* dc_dev /*or NULL*/, void* stream);
int hipnlp_pose_kkt_diag_precond_device(hipnlp_pose_handle* h, const double* hess_values_dev, const double* jac_values_dev, double* minv_top_dev /*[batch][81]*/,
                                        double* minv_bottom_dev /*[batch][m]*/, const double* dx_dev /*or NULL*/, const double* dc_dev /*or NULL*/, double floor,
                                        void* stream);
int hipnlp_pose_kkt_minres_device(hipnlp_pose_handle* h, const double* hess_values_dev, const double* jac_values_dev, const double* rhs_top_dev,
                                  const double* rhs_bottom_dev, double* sol_top_dev, double* sol_bottom_dev, int32_t* iterations_dev, double* residual_dev,
                                  int32_t* status_dev, const double* dx_dev /*or NULL*/, const double* dc_dev /*or NULL*/, const double* minv_top_dev /*or NULL*/,
                                  const double* minv_bottom_dev /*or NULL*/, int build_diagonal, double floor, double rtol, int max_iterations, void* stream);

/* The dense L D L^T factorisation of the same K = [[H + diag d_x + delta I, J^T], [J, -diag d_c]] per pose, with its INERTIA, a
 * regularisation ladder and the solves — what an interior-point step needs and MINRES cannot give.  The order N = 81 + m is at most 176:
 * one workgroup holds the packed lower triangle (N (N + 1) / 2 doubles) in its LDS, assembles it from the two stored value runs, factors
 * it by Bunch-Kaufman partial pivoting (the algorithm of LAPACK's unblocked DSPTF2('L'): 1x1 and 2x2 pivots, alpha = (1 + sqrt 17) / 8),
 * reads the inertia off D and solves.  Each call is ONE launch on a grid of `batch` workgroups of 1 024 threads, enqueued on `stream`
 * (NULL: the handle's own), not synchronised; no workspace, nothing owned by the handle: calls on different streams are independent.
 * Every element of the factor and of a solution is one fixed chain of fused multiply-adds (hippopt_amd/csrc/pose_ldl.h): the same bits on
 * every launch, at every batch position.
 *   hipnlp_pose_kkt_ldl_doubles       N (N + 1) / 2, the doubles of one pose's packed factor
 *   hipnlp_pose_kkt_ldl_device        assemble, factor, count, climb the ladder, then nrhs solves (0 <= nrhs <= 8; right-hand sides
 *                                     [batch][nrhs][81] and [batch][nrhs][m], solutions alike; all four NULL with nrhs == 0).
 *                                     inertia_dev [batch][3] int32: positive, negative, zero eigenvalues.  status_dev [batch] int32:
 *                                     0 factored (and, with a ladder, the inertia is (81, m, 0)); 1 exactly singular: a pivot column of
 *                                     zeros, counted as ONE zero, the factorisation ends there; 2 data that is not finite; 3 the ladder
 *                                     is exhausted.  The ladder (IPOPT's inertia correction, top block only): try 0 has delta = 0, try
 *                                     t >= 1 has delta_1 = delta_init, delta_(t+1) = delta_t * kappa added to the 81 diagonal elements of
 *                                     the top block on a re-assembly; it ends at the first try with inertia (81, m, 0), at status 2, or
 *                                     at try max_tries (<= 16); max_tries == 0: factor once, report the inertia as it is.  Status,
 *                                     inertia, factor and solutions are those of the last try; delta_dev [batch] its delta and tries_dev
 *                                     [batch] int32 its number (either may be NULL).  With status 1 or 2 the solutions are NaN.
 *                                     factor_dev [batch][doubles] and pivots_dev [batch][N] int32 (both or neither) receive the factor:
 *                                     D and the multipliers in the packed lower triangle, the pivot vector in LAPACK's convention
 *                                     (1-based; k > 0: a 1x1 pivot; a pair of -k: a 2x2 pivot) — the values of DSPTF2, but EVERY
 *                                     interchange is applied to whole rows of L (P K P^T = L D L^T), which DSPTRS would not expect.
 *   hipnlp_pose_kkt_ldl_solve_device  nrhs (1 .. 8) solves from a stored factor and pivot vector: no assembly, no value run read; the
 *                                     bits of the solves of the call that stored them.
 * HIPNLP_E_INVALID: a null handle or required pointer, nrhs out of range, one of factor_dev / pivots_dev alone, max_tries outside
 * 0 .. 16, and with max_tries > 0 a delta_init that is not a finite number > 0 or a kappa that is not a finite number > 1.
 * HIPNLP_E_UNSUPPORTED: the handle's pattern is beyond hipnlp_pose_kkt_times_device's caps or 81 + m > 176.  Measured:
 * profiles/r15_pose_ldl.txt (tools/pose_ldl_probe.py) — 0.24 x torch.linalg.solve on the dense K, slower than MINRES at dx, dc in U[1, 2].
 * Both launches: replayable from a captured graph after one eager call on the handle (tests/test_gpu_graph_replay.py). */
int hipnlp_pose_kkt_ldl_doubles(const hipnlp_pose_handle* h);
int hipnlp_pose_kkt_ldl_device(hipnlp_pose_handle* h, const double* hess_values_dev, const double* jac_values_dev, const double* dx_dev /*or NULL*/,
                               const double* dc_dev /*or NULL*/, int nrhs, const double* rhs_top_dev, const double* rhs_bottom_dev, double* sol_top_dev,
                               double* sol_bottom_dev, int32_t* inertia_dev /*[batch][3]*/, int32_t* status_dev /*[batch]*/, double* delta_dev /*or NULL*/,
                               int32_t* tries_dev /*or NULL*/, double delta_init, double kappa, int max_tries, double* factor_dev /*or NULL*/,
                               int32_t* pivots_dev /*or NULL*/, void* stream);
int hipnlp_pose_kkt_ldl_solve_device(hipnlp_pose_handle* h, const double* factor_dev, const int32_t* pivots_dev, int nrhs, const double* rhs_top_dev,
                                     const double* rhs_bottom_dev, double* sol_top_dev, double* sol_bottom_dev, void* stream);
int hipnlp_pose_cost_terms(hipnlp_pose_handle* h, double* values /*[batch][HIPNLP_POSE_NCOST_TERMS]*/);
const char* hipnlp_pose_cost_term_name(int i);
int hipnlp_pose_num_row_blocks(const hipnlp_pose_handle* h);
int hipnlp_pose_row_block(const hipnlp_pose_handle* h, int i, const char** name, int32_t* first_row, int32_t* rows);
/* kernel duration of the last host-buffer call by HIP events — only for calls made with the timing ON (off by default since round 5: the
 * two event records drain the stream around the launch, ~3 us of a 25 us call for one pose) */
int hipnlp_pose_set_host_timing(hipnlp_pose_handle* h, int on);
int hipnlp_pose_last_kernel_ms(hipnlp_pose_handle* h, float* ms);

#ifdef __cplusplus
}
#endif
#endif /* HIPNLP_H */
