/*
 * nmpc_amd.h -- C-ABI of the MI355X-native batched NMPC solve step.
 *
 * Drop-in boundary for the per-timestep NLP of devsonni/MPC-Implementation
 * (Python/NMPC_TT.py).  The reference builds the NLP symbolically and solves
 * one scenario per call:
 *
 *   solver = ca.nlpsol('solver', 'ipopt', nlp_prob, opts)      Python/NMPC_TT.py:267
 *   sol = solver(x0=, lbx=, ubx=, lbg=, ubg=, p=)              Python/NMPC_TT.py:358-365
 *   u = ca.reshape(sol['x'], n_controls, N)                    Python/NMPC_TT.py:367
 *   ff_value = ff(u, args['p'])                                Python/NMPC_TT.py:368
 *
 * This library replaces that pair with a handle created from a structured
 * problem description (nmpc_create <- nlpsol) and a batched call
 * (nmpc_solve_batch <- solver(...)), B independent scenarios per call, all
 * solved on one MI355X by hand-written HIP kernels (one wavefront per
 * scenario).  Plain pointers and sizes only.
 *
 * Layouts (match CasADi's DM column vectors / Function.map horzcat):
 *   x0, lbx, ubx, x_out, lam_x_out : nw x B column-major, nw = 6*N   (w = vec(U), U is 6 x N)
 *   lbg, ubg, g_out, lam_g_out     : ng x B column-major, ng = (5+n_obs)*(N+1)
 *   p                              : np x B column-major, p = [x0(8); xs(3); dynamic obstacle coords]
 *   X_out                          : 8*(N+1) x B column-major  (ff(u, p), Python/NMPC_TT.py:169)
 *   lam_p_out                      : np x B column-major, -grad_p (f + lam_g' g) at x_out
 *                                    (CasADi nlpsol's lam_p; nullable)
 * A leading dimension of 0 broadcasts one column to every scenario (bounds
 * are normally shared: Python/NMPC_TT.py:269-306).  +-inf (|b| >= 1e19)
 * means "no bound", as ca.inf does (Python/NMPC_TT.py:280-282).
 *
 * Errors: functions return 0 on success and a negative NMPC_E* code on
 * invalid arguments or a HIP failure; nmpc_last_error() gives the message.
 * Non-convergence is NOT an error (the reference never checks it):
 * it is reported per scenario in status[] with IPOPT's ApplicationReturnStatus
 * codes (Ipopt::Solve_Succeeded = 0, Solved_To_Acceptable_Level = 1,
 * Infeasible_Problem_Detected = 2, Search_Direction_Becomes_Too_Small = 3,
 * Maximum_Iterations_Exceeded = -1,
 * Restoration_Failed = -2, Error_In_Step_Computation = -3,
 * Invalid_Number_Detected = -13).
 *
 * Threading/ownership: a handle is not thread-safe (one per GPU/stream).  The
 * caller owns every buffer; nothing is retained past a call.  The handle owns
 * its device workspace, grown on demand.
 */
#ifndef NMPC_AMD_H
#define NMPC_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NMPC_MAX_OBS 16
#define NMPC_MAX_N 63

enum {
  NMPC_OK = 0,
  NMPC_E_INVALID = -1, /* bad descriptor / argument */
  NMPC_E_HIP = -2,     /* HIP runtime failure */
  NMPC_E_NOMEM = -3    /* device allocation failed */
};

enum {
  NMPC_MODEL_UAV8G = 0, /* 8 states / 6 controls, Python/NMPC_TT.py:94-151; p = [x0(8); xs(3); ...] */
  NMPC_MODEL_UAV5 = 1   /* no gimbal: 5 states / 3 controls, distance cost, rows [z, theta] (+ obstacles),
                           MATLAB/Dynamic Obstacles/NMPC_TT.m:26-35,102-111,129-134; w = vec(U) with U
                           3 x N, p = [x0(5); xs(3); ...], X_out 5 x (N+1); w2 is ignored.
                           All entry points, including nmpc_shift_dev / nmpc_closed_loop_dev */
};

/* IPOPT options honoured by the solver (names and meaning as IPOPT's;
 * nmpc_default_options() fills IPOPT's defaults, the reference overrides
 * max_iter=100, acceptable_tol=1e-8, acceptable_obj_change_tol=1e-6 at
 * Python/NMPC_TT.py:257-265). */
typedef struct nmpc_options {
  int32_t max_iter, acceptable_iter, max_soc, max_soft_resto_iters;
  /* watchdog procedure of the backtracking line search (IPOPT defaults 10 and 3;
   * a trigger of 0 disables it) */
  int32_t watchdog_shortened_iter_trigger, watchdog_trial_iter_max;
  /* not an IPOPT option: 1 = Riccati factorisation and solves in fp32 (the fp32 leg of
   * BASELINE config 5's fp32-vs-fp64 sweep); the iterate, residuals, line search and
   * termination tests stay fp64.  0 (default) = fp64 throughout. */
  int32_t linear_solver_fp32, reserved0;
  double tol, acceptable_tol, acceptable_obj_change_tol, acceptable_dual_inf_tol;
  double acceptable_constr_viol_tol, acceptable_compl_inf_tol;
  double dual_inf_tol, constr_viol_tol, compl_inf_tol;
  double mu_init, kappa_mu, theta_mu, barrier_tol_factor, tau_min;
  double bound_push, bound_frac, slack_bound_push, slack_bound_frac, bound_relax_factor;
  double bound_mult_init_val, constr_mult_init_max;
  double nlp_scaling_max_gradient, nlp_scaling_min_value, kappa_d, kappa_sigma, s_max;
  double theta_max_fact, theta_min_fact, gamma_theta, gamma_phi, delta, s_theta, s_phi, eta_phi;
  double alpha_red_factor, alpha_min_frac, kappa_soc, obj_max_inc;
  double first_hessian_perturbation, min_hessian_perturbation, max_hessian_perturbation;
  double perturb_inc_fact_first, perturb_inc_fact, perturb_dec_fact;
  double tiny_step_tol, soft_resto_pderror_reduction_factor;
  /* feasibility restoration phase */
  double resto_penalty_parameter, resto_proximity_weight, required_infeasibility_reduction;
  double bound_mult_reset_threshold, constr_mult_reset_threshold;
} nmpc_options;

/* Structured replacement for the symbolic nlp_prob of Python/NMPC_TT.py:247-255. */
typedef struct nmpc_desc {
  int32_t model;    /* NMPC_MODEL_UAV8G */
  int32_t N;        /* horizon, 1..NMPC_MAX_N (reference: 15, Python/NMPC_TT.py:58) */
  int32_t np;       /* length of p, >= 11 */
  int32_t n_obs;    /* 0..NMPC_MAX_OBS obstacle rows per stage */
  double T;         /* Euler step (Python/NMPC_TT.py:57; 0.2 in 10_obstacles.py:95) */
  double w1, w2;    /* cost weights (Python/NMPC_TT.py:204-205) */
  double vfov, hfov;/* FOV angles (Python/NMPC_TT.py:201-202) */
  double obs_x[NMPC_MAX_OBS], obs_y[NMPC_MAX_OBS];
  double obs_rsum[NMPC_MAX_OBS];      /* UAV_r + obs_r (Python/NMPC_TT.py:230-231) */
  int32_t obs_x_pidx[NMPC_MAX_OBS];   /* -1 = constant, else index into p (dynamic obstacles) */
  int32_t obs_y_pidx[NMPC_MAX_OBS];
  nmpc_options opts;
  /* cost weights from p (batched weight sweep; the RL replay of
   * MATLAB/Race Track 1/MPC.m:1,127 rebuilds nlpsol per weight pair): index
   * into p, or -1 to use w1 / w2 above */
  int32_t w1_pidx, w2_pidx;
} nmpc_desc;

typedef struct nmpc_handle nmpc_handle;

/* Fill IPOPT's default option values. */
void nmpc_default_options(nmpc_options* opts);

/* Replaces ca.nlpsol('solver', 'ipopt', nlp_prob, opts) (Python/NMPC_TT.py:267).
 * Binds the current HIP device. */
int nmpc_create(const nmpc_desc* desc, nmpc_handle** out);
int nmpc_destroy(nmpc_handle* h);

/* Problem dimensions: nw = nu N, ng = (nb+n_obs)(N+1), np, nX = nx(N+1)
 * (gimbal model: nu = 6, nb = 5, nx = 8; no-gimbal model: nu = 3, nb = 2, nx = 5). */
int nmpc_dims(const nmpc_handle* h, int32_t* nw, int32_t* ng, int32_t* np, int32_t* nX);

/* Replaces sol = solver(x0=, lbx=, ubx=, lbg=, ubg=, p=) (Python/NMPC_TT.py:358-365)
 * for B scenarios at once.  HOST pointers; synchronous.  Output pointers other
 * than x_out may be NULL.
 * Bounds as IPOPT reads them: |b| >= 1e19 is no bound; lbx == ubx fixes a variable
 * (fixed_variable_treatment = make_parameter: held at the bound, no step, lam_x 0);
 * rows with lbg == ubg are IPOPT's equality constraints c(x) = g(x) - lbg = 0 (no slack,
 * no relaxation; augmented-system step with IPOPT's inertia test), up to 128
 * per scenario.  A batch with any equality row runs on the equality class (global rows,
 * any shape, ~850 KB of device workspace per scenario): this host-pointer entry point scans
 * the bounds on the host, allocates that workspace when the batch needs it and launches
 * the one class that applies.
 * lbx > ubx, more than 128 equality rows, or equality rows with the fp32 Riccati leg
 * report status -11 (IPOPT Invalid_Problem_Definition) for that scenario. */
int nmpc_solve_batch(nmpc_handle* h, int32_t B,
                     const double* x0, int64_t ld_x0,
                     const double* lbx, int64_t ld_lbx, const double* ubx, int64_t ld_ubx,
                     const double* lbg, int64_t ld_lbg, const double* ubg, int64_t ld_ubg,
                     const double* p, int64_t ld_p,
                     double* x_out, double* f_out, double* g_out,
                     double* lam_x_out, double* lam_g_out, double* lam_p_out, double* X_out,
                     int32_t* status, int32_t* iters);

/* Same with DEVICE pointers, enqueued on `stream` (hipStream_t; NULL = default
 * stream); returns without synchronising (no host round trip: once the handle's workspace
 * covers B, a call only enqueues kernels).  Outputs other than x_out may be NULL.
 * Equality rows: the bounds are scanned on the device and a device flag lets exactly one
 * of the problem's class and the equality class run.  The equality class needs its
 * workspace reserved for B scenarios beforehand (nmpc_reserve_eq); without it a batch that
 * has equality rows is not solved and every scenario reports NMPC_STATUS_EQ_UNRESERVED
 * with iters 0 and NaN in f and in every output vector passed (x_out, g_out, lam_x_out,
 * lam_g_out, lam_p_out, X_out), so none keeps an earlier call's values.  Batches without
 * equality rows need no reservation. */
int nmpc_solve_batch_dev(nmpc_handle* h, int32_t B,
                         const double* x0, int64_t ld_x0,
                         const double* lbx, int64_t ld_lbx, const double* ubx, int64_t ld_ubx,
                         const double* lbg, int64_t ld_lbg, const double* ubg, int64_t ld_ubg,
                         const double* p, int64_t ld_p,
                         double* x_out, double* f_out, double* g_out,
                         double* lam_x_out, double* lam_g_out, double* lam_p_out, double* X_out,
                         int32_t* status, int32_t* iters, void* stream);

/* Per-scenario status of a device-pointer call (nmpc_solve_batch_dev, nmpc_closed_loop_dev)
 * whose batch has equality rows (lbg == ubg) while the equality class's workspace does not
 * cover B: the batch was not solved (IPOPT's Insufficient_Memory code).  Reserve first. */
#define NMPC_STATUS_EQ_UNRESERVED (-102)
/* Allocate the equality class's device workspace for B scenarios (synchronous, like any
 * allocation; a no-op when it already covers B or for the fp32 leg, whose equality rows
 * report -11).  The _dev entry points never allocate it themselves, so that they never
 * synchronise the host; nmpc_solve_batch allocates it on demand. */
int nmpc_reserve_eq(nmpc_handle* h, int32_t B);

/* Evaluation of the NLP's function layer at GIVEN points, for B scenarios at once: CasADi's
 * nlp_f / nlp_g / nlp_grad_f of an nlpsol object and ff(u, p) of Python/NMPC_TT.py:368, plus
 * a first-order (KKT) certificate that does not come from the solver.  x is any decision
 * vector (a policy's output, a perturbed or shifted plan, a solve's x_out).  No options,
 * problem classes or statuses are involved; non-finite inputs give non-finite outputs.
 *
 * DEVICE pointers, enqueued on `stream`; never synchronises and allocates nothing once the
 * handle's workspace covers B (the solve's workspace serves: a handle that has solved a
 * batch of B evaluates B without allocating).  Layouts, leading-dimension-0 broadcast and
 * |b| >= 1e19 = no bound exactly as nmpc_solve_batch.
 *   x (nw x B) and p (np x B) are required.
 *   lam_g (ng x B), lam_x (nw x B): multipliers in CasADi's sign convention (at a solution
 *     grad f + J_g^T lam_g + lam_x = 0, lam > 0 on an upper bound); NULL = zeros.
 *   lbx, ubx, lbg, ubg: only kkt_out reads them; NULL unless kkt_out is given.
 * Every output may be NULL, at least one must not be:
 *   f_out (B), g_out (ng x B), X_out (nx(N+1) x B) as nmpc_solve_batch's;
 *   grad_f_out (nw x B) = grad_w f;
 *   grad_l_out (nw x B) = grad_w f + J_g^T lam_g + lam_x (== grad_f_out bitwise without
 *     multipliers);
 *   kkt_out (5 x B), unnormalised, per scenario
 *     [0] stat  = |grad_l|_inf
 *     [1] gmax  = |grad_f|_inf
 *     [2] viol  = max(0, g - ubg, lbg - g, x - ubx, lbx - x) over the bounds present
 *     [3] compl = max over rows and variables of |lam| * gap, the gap taken towards the upper
 *                 bound where lam > 0 and towards the lower bound where lam < 0; a multiplier
 *                 that points at an absent bound contributes 0
 *     [4] lmax  = max(|lam_g|_inf, |lam_x|_inf)
 *     (a NaN in any term makes that entry NaN).  IPOPT's unscaled acceptance test read on
 *     g(x) is stat <= dual_inf_tol, viol <= constr_viol_tol, compl <= compl_inf_tol (1 + lmax).
 * f sums the stages 0..N-1; stage 0 is constant in w, so its derivative terms are
 * structurally absent (with N = 1, grad_f is exactly 0).  Fixed variables and equality rows
 * need no special case: the bounds only enter viol and compl.
 * B <= 0, a NULL x or p, every output NULL, kkt_out with a bound missing, or a leading
 * dimension that is neither 0 nor >= the vector length return NMPC_E_INVALID before any
 * device call. */
int nmpc_eval_batch_dev(nmpc_handle* h, int32_t B,
                        const double* x, int64_t ld_x, const double* p, int64_t ld_p,
                        const double* lam_g, int64_t ld_lam_g, const double* lam_x, int64_t ld_lam_x,
                        const double* lbx, int64_t ld_lbx, const double* ubx, int64_t ld_ubx,
                        const double* lbg, int64_t ld_lbg, const double* ubg, int64_t ld_ubg,
                        double* f_out, double* g_out, double* X_out,
                        double* grad_f_out, double* grad_l_out, double* kkt_out, void* stream);

/* Same with HOST pointers; synchronous (staged through the handle's device buffer). */
int nmpc_eval_batch(nmpc_handle* h, int32_t B,
                    const double* x, int64_t ld_x, const double* p, int64_t ld_p,
                    const double* lam_g, int64_t ld_lam_g, const double* lam_x, int64_t ld_lam_x,
                    const double* lbx, int64_t ld_lbx, const double* ubx, int64_t ld_ubx,
                    const double* lbg, int64_t ld_lbg, const double* ubg, int64_t ld_ubg,
                    double* f_out, double* g_out, double* X_out,
                    double* grad_f_out, double* grad_l_out, double* kkt_out);

/* Jacobian- and Hessian-vector products at GIVEN decision vectors, for a whole batch: the
 * second-order half of the function layer (CasADi's nlp_jac_g and nlp_hess_l applied to
 * vectors).  For each of B scenarios and each of nv >= 1 directions v_d in decision space
 * (nw long, the model's own layout):
 *   jv_out (ng nv x B) = J_g(x, p) v_d
 *   hv_out (nw nv x B) = (obj_factor grad^2_w f + sum_i lam_g_i grad^2_w g_i) v_d
 *                        (CasADi's hess_l convention; lam_g in CasADi's sign convention as in
 *                        nmpc_eval_batch, NULL = zeros; obj_factor is shared by the batch)
 *   dX_out (nx(N+1) nv x B) = (dX/dw) v_d, the tangent of the rollout in X_out's layout;
 *                        stage 0 is exactly 0.
 * Within a scenario direction d occupies [d n, (d+1) n) of each array.  v is nw nv per
 * scenario; ld_v = 0 shares one set of directions with every scenario (ld_v = 0 and v = I give
 * the dense J_g and Hessian).  x, p and lam_g follow nmpc_eval_batch_dev's leading-dimension
 * rules.  Every output may be NULL, at least one must not be.  No bounds, options, classes or
 * statuses are involved.  Non-finite input gives non-finite output only in the directions and
 * scenarios it touches: directions are independent of each other.  Stage 0 is constant in w,
 * so its terms are structurally absent (with N = 1 only the last stage's row curvature
 * contributes to the Hessian).
 * DEVICE pointers, enqueued on `stream`; never synchronises, and allocates nothing once the
 * handle's workspace covers B (a solve's workspace does).
 * A NULL handle, B <= 0, nv <= 0, a NULL x, p or v, every output NULL, or a leading dimension
 * that is neither 0 nor >= the vector length (nw nv for v) return NMPC_E_INVALID before any
 * device call. */
int nmpc_products_batch_dev(nmpc_handle* h, int32_t B, int32_t nv,
                            const double* x, int64_t ld_x, const double* p, int64_t ld_p,
                            const double* lam_g, int64_t ld_lam_g, double obj_factor,
                            const double* v, int64_t ld_v,
                            double* jv_out, double* hv_out, double* dX_out, void* stream);

/* Same with HOST pointers; synchronous (staged through the handle's device buffer). */
int nmpc_products_batch(nmpc_handle* h, int32_t B, int32_t nv,
                        const double* x, int64_t ld_x, const double* p, int64_t ld_p,
                        const double* lam_g, int64_t ld_lam_g, double obj_factor,
                        const double* v, int64_t ld_v,
                        double* jv_out, double* hv_out, double* dX_out);

/* Solves with the condensed KKT matrix at GIVEN decision vectors, for a whole batch: the
 * Newton-step operator of the interior-point method (the solver's Riccati factorisation, its
 * solves and its inertia verdict) as a function of its own.  For each of B scenarios, at x
 * with parameters p, multipliers lam_g (CasADi's sign convention, NULL = zeros) and
 * obj_factor (shared by the batch),
 *   M  = W + diag(sigma_x) + delta I + J^T diag(sigma_s + delta) J
 *   W  = obj_factor grad^2_w f + sum_i lam_g_i grad^2_w g_i      (nmpc_products_batch's hv)
 *   M dw_d = r_w,d + J^T r_g,d                                   for each of nr >= 1 right-hand sides
 * i.e. IPOPT's primal-dual system with the slacks and bound multipliers eliminated; delta is
 * the primal regularisation delta_w, which enters the slack block too.  M is unscaled (unit
 * row scaling, objective factor = obj_factor).
 *   sigma_x (nw x B), NULL = zeros: the variables' barrier weights.  +inf marks a fixed
 *     variable: its row and column leave the system and dw is exactly 0 there.
 *   sigma_s (ng x B), NULL = zeros: the rows' (slacks') barrier weights, finite.
 *   delta (B), NULL = 0; ld_delta = 0 shares one value.
 *   r_w (nw nr per scenario), r_g (ng nr per scenario): either may be NULL (= zeros), not both;
 *     right-hand side d occupies [d n, (d+1) n).  A leading dimension of 0 shares one set with
 *     every scenario, as for sigma_x and sigma_s.
 * x, p and lam_g follow nmpc_products_batch_dev's leading-dimension rules.
 *   dw_out  (nw nr x B)        = dw_d
 *   dX_out  (nx(N+1) nr x B)   = (dX/dw) dw_d, the state step; stage 0 is exactly 0
 *   jdw_out (ng nr x B)        = J dw_d (the row step: ds = J dw - r_d, dlam_g = sigma_s ds ...)
 *   info_out (B x int32): 0 = factorised and every Riccati pivot positive definite (IPOPT's
 *     inertia test: M is positive definite); 1 = wrong inertia or singular; -11 = invalid
 *     weights (a negative or NaN sigma_x / sigma_s / delta, an infinite sigma_s or delta).
 *     With 1 or -11 that scenario's other outputs are NaN, never a step from a failed factor.
 * Each output may be NULL, at least one of dw_out, dX_out, jdw_out must not be.  Stage 0's
 * rows have a zero Jacobian: their sigma_s and r_g entries are never read.  The right-hand
 * sides are independent: a non-finite one gives a non-finite column of its own only.  The
 * no-gimbal model's absent controls are not part of the system (nw = 3N).  An infinite
 * sigma_s (an equality row) is not supported here.
 * DEVICE pointers, enqueued on `stream`; never synchronises, and allocates nothing once the
 * handle's workspace covers B (a solve's workspace does).  One wavefront per scenario forms
 * every right-hand side: the factorisation is done once.
 * A NULL handle, B <= 0, nr <= 0, a NULL x or p, both right-hand sides NULL, dw_out, dX_out
 * and jdw_out all NULL, or a leading dimension that is neither 0 nor >= the vector length
 * return NMPC_E_INVALID before any device call. */
int nmpc_kkt_solve_batch_dev(nmpc_handle* h, int32_t B, int32_t nr,
                             const double* x, int64_t ld_x, const double* p, int64_t ld_p,
                             const double* lam_g, int64_t ld_lam_g, double obj_factor,
                             const double* sigma_x, int64_t ld_sigma_x,
                             const double* sigma_s, int64_t ld_sigma_s,
                             const double* delta, int64_t ld_delta,
                             const double* r_w, int64_t ld_r_w, const double* r_g, int64_t ld_r_g,
                             double* dw_out, double* dX_out, double* jdw_out, int32_t* info_out,
                             void* stream);

/* Same with HOST pointers; synchronous (staged through the handle's device buffer). */
int nmpc_kkt_solve_batch(nmpc_handle* h, int32_t B, int32_t nr,
                         const double* x, int64_t ld_x, const double* p, int64_t ld_p,
                         const double* lam_g, int64_t ld_lam_g, double obj_factor,
                         const double* sigma_x, int64_t ld_sigma_x,
                         const double* sigma_s, int64_t ld_sigma_s,
                         const double* delta, int64_t ld_delta,
                         const double* r_w, int64_t ld_r_w, const double* r_g, int64_t ld_r_g,
                         double* dw_out, double* dX_out, double* jdw_out, int32_t* info_out);

/* Parameter-direction products at GIVEN points, for a whole batch: the parameter half of the
 * function layer.  With L = obj_factor f + lam_g^T g (lam_g in CasADi's sign convention,
 * NULL = zeros; obj_factor shared by the batch), for each of B scenarios and each of nd >= 0
 * directions dp_d in parameter space (np long, the model's own layout [x0(nx); xt, yt, .; ...]):
 *   jp_out  (ng nd x B)        = (dg/dp) dp_d; stage 0's rows are not zero here
 *   hp_out  (nw nd x B)        = (d_p grad_w L) dp_d, the parameter tangent of nmpc_eval_batch's
 *                                grad_l (lam_x absent) at fixed (x, lam_g)
 *   dXp_out (nx(N+1) nd x B)   = (dX/dp) dp_d in X_out's layout; stage 0 is exactly dp_d[0:nx]
 *   gp_out  (np x B)           = grad_p L, independent of the directions; with obj_factor = 1 at
 *                                a solve's (x, lam_g) it is the negative of that solve's lam_p.
 * The derivatives are exact (no difference step): the initial state through the tangent of the
 * rollout and the Lagrangian adjoint, the target through the stage costs, an obstacle centre
 * taken from p through that obstacle's rows, a cost weight taken from p through the cost term it
 * scales.  An entry of p that nothing reads -- the target's third entry, a tail entry no
 * obstacle or weight index names -- gives exactly 0 in gp_out, and its entry of dp is never
 * read.
 * Within a scenario direction d occupies [d n, (d+1) n) of each array.  dp is np nd per
 * scenario; ld_dp = 0 shares one set of directions with every scenario (ld_dp = 0 and dp = I
 * give the dense dg/dp and d_p grad_w L).  x, p and lam_g follow nmpc_products_batch_dev's
 * leading-dimension rules.  Every output may be NULL, at least one must not be.  nd = 0 is
 * allowed with gp_out alone: dp and the three directional outputs must then be NULL.
 * Directions are independent of each other: a non-finite entry of dp gives non-finite output in
 * its own direction only, and gp_out depends on no direction.  The no-gimbal model has nx = 5
 * and nw = 3N.
 * DEVICE pointers, enqueued on `stream`; never synchronises, and allocates nothing once the
 * handle's workspace covers B (a solve's workspace does).
 * A NULL handle, B <= 0, nd < 0, a NULL x or p, every output NULL, a directional output with
 * nd = 0 or a NULL dp, a non-NULL dp with nd = 0, or a leading dimension that is neither 0 nor
 * >= the vector length (np nd for dp) return NMPC_E_INVALID before any device call. */
int nmpc_param_products_batch_dev(nmpc_handle* h, int32_t B, int32_t nd,
                                  const double* x, int64_t ld_x, const double* p, int64_t ld_p,
                                  const double* lam_g, int64_t ld_lam_g, double obj_factor,
                                  const double* dp, int64_t ld_dp,
                                  double* jp_out, double* hp_out, double* dXp_out, double* gp_out,
                                  void* stream);

/* Same with HOST pointers; synchronous (staged through the handle's device buffer). */
int nmpc_param_products_batch(nmpc_handle* h, int32_t B, int32_t nd,
                              const double* x, int64_t ld_x, const double* p, int64_t ld_p,
                              const double* lam_g, int64_t ld_lam_g, double obj_factor,
                              const double* dp, int64_t ld_dp,
                              double* jp_out, double* hp_out, double* dXp_out, double* gp_out);

/* Adjoint (vector-Jacobian) products at GIVEN points, for a whole batch: the transposed half of
 * the function layer, what reverse-mode differentiation of anything built on g, grad_w L or X
 * needs (a loss on the applied control pulled back to cost weights from p -- the reference's
 * replay over weight pairs at w1_pidx --, to obstacle centres, to the initial state).  With
 * L = obj_factor f + lam_g^T g (lam_g in CasADi's sign convention, NULL = zeros; obj_factor
 * shared by the batch) and W = obj_factor grad^2 f + sum_i lam_g_i grad^2 g_i, for each of B
 * scenarios and each of na >= 1 seeds (y_d on g, z_d on grad_w L, Xb_d on X):
 *   wbar_out (nw na x B) = J_g^T y_d + W z_d + (dX/dw)^T Xb_d
 *   pbar_out (np na x B) = (dg/dp)^T y_d + (d_p grad_w L)^T z_d + (dX/dp)^T Xb_d
 * the transposes of nmpc_products_batch_dev's and nmpc_param_products_batch_dev's maps, formed
 * exactly by one forward tangent (z alone needs it) and one reverse sweep per seed, never as
 * matrices.  y is ng na per scenario, z nw na, Xb nx(N+1) na in X_out's layout; each of the
 * three may be NULL and then contributes nothing (its term is not formed), at least one must
 * not be.  Stage 0's entries of y and Xb are read: (dg/dp) and (dX/dp) have stage-0 rows, and
 * with Xb alone the x0 block of pbar receives Xb's stage 0 once.  An entry of p that nothing
 * reads gives exactly 0 in pbar_out.  The gradients of f itself are nmpc_eval_batch's
 * grad_f_out and nmpc_param_products_batch's gp_out and are not repeated here.
 * Within a scenario seed d occupies [d n, (d+1) n) of each array; a leading dimension of 0
 * shares one set of seeds with every scenario.  x, p and lam_g follow
 * nmpc_products_batch_dev's leading-dimension rules.  Either output may be NULL, not both.
 * Seeds are independent of each other: a non-finite entry of one seed gives non-finite output
 * for that seed only.  The no-gimbal model has nx = 5 and nw = 3N.
 * DEVICE pointers, enqueued on `stream`; never synchronises, and allocates nothing once the
 * handle's workspace covers B (a solve's workspace does).
 * A NULL handle, B <= 0, na <= 0, a NULL x or p, y, z and Xb all NULL, both outputs NULL, or a
 * leading dimension that is neither 0 nor >= the vector length (ng na, nw na, nx(N+1) na for
 * the seeds) return NMPC_E_INVALID before any device call. */
int nmpc_adjoint_products_batch_dev(nmpc_handle* h, int32_t B, int32_t na,
                                    const double* x, int64_t ld_x, const double* p, int64_t ld_p,
                                    const double* lam_g, int64_t ld_lam_g, double obj_factor,
                                    const double* y, int64_t ld_y, const double* z, int64_t ld_z,
                                    const double* Xb, int64_t ld_Xb,
                                    double* wbar_out, double* pbar_out, void* stream);

/* Same with HOST pointers; synchronous (staged through the handle's device buffer). */
int nmpc_adjoint_products_batch(nmpc_handle* h, int32_t B, int32_t na,
                                const double* x, int64_t ld_x, const double* p, int64_t ld_p,
                                const double* lam_g, int64_t ld_lam_g, double obj_factor,
                                const double* y, int64_t ld_y, const double* z, int64_t ld_z,
                                const double* Xb, int64_t ld_Xb,
                                double* wbar_out, double* pbar_out);

/* Reverse-mode sensitivity of a SOLUTION, for a whole batch, in one launch: what a backward pass
 * through the solve needs, with nothing on the host.  At a solve's x* (x), its multipliers
 * lam_g*, lam_x* (CasADi's signs: negative towards the lower bound) and parameters p, with
 * L = f + lam_g^T g, W = grad^2_w L, J = dg/dw, and the barrier weights of the point
 *   sigma = max(-lam, 0) / max(v - lo, eps_lo) + max(lam, 0) / max(hi - v, eps_hi),
 *   eps_b = bound_relax_factor max(1, |b|)   (the handle's option),
 * Sigma_x from (x, lam_x, lbx, ubx) and Sigma_s from (g, lam_g, lbg, ubg), the condensed matrix
 *   M = W + diag(Sigma_x) + delta I + J^T diag(Sigma_s + delta) J
 * is factorised once per scenario, at delta = 0 where its inertia is right and otherwise along
 * IPOPT's inertia-correction ladder (first_hessian_perturbation, then x perturb_inc_fact_first,
 * then x perturb_inc_fact, while <= max_hessian_perturbation; the handle's options).  For each of
 * na >= 1 seeds (x_bar_d on x*, lam_g_bar_d on lam_g*, X_bar_d on the state trajectory X*):
 *   q_out    (nw na x B) = M^-1 (x_bar_d + (dX/dw)^T X_bar_d + J^T Sigma_s lam_g_bar_d)
 *   jq_out   (ng na x B) = J q; stage 0's rows are exactly 0
 *   pbar_out (np na x B) = -(d_p grad_w L)^T q + (dg/dp)^T Sigma_s (lam_g_bar_d - J q)
 *                          + (dX/dp)^T X_bar_d
 * so that <pbar, dp> = <x_bar, dx*> + <lam_g_bar, dlam_g*> + <X_bar, dX*> for every direction dp
 * of the parameters, with (dx*, dlam_g*) the interior-point linearisation of the optimality
 * conditions at the point.  info_out (B): 0 = factorised with the right inertia; 1 = no rung of
 * the ladder did; -11 = an equality row (lbg == ubg, which needs the augmented system), lbx > ubx,
 * or a weight that is not a finite non-negative number (a NaN multiplier).  With 1 or -11 the
 * scenario's pbar, q and jq are NaN and its neighbours are untouched.  delta_out (B): the delta
 * of the last factorisation tried (0 with -11).
 * g is the row values the weights are taken at (a solve's g_out); NULL = the kernel's own
 * g(x, p).  A variable with lbx == ubx is fixed: it leaves the system, its x_bar is ignored
 * and its q is exactly 0.  A bound beyond +-1e19 enters the formula as it stands: its slack is of
 * that size and its term vanishes to rounding.  An entry of p that nothing reads gives exactly 0
 * in pbar_out.
 * Within a scenario seed d occupies [d n, (d+1) n) of each seed and output array; X_bar is
 * nx(N+1) na in X_out's layout.  Each seed may be NULL and then contributes nothing, at least one
 * must not be.  x, p, lam_g, lam_x, g and the bounds are n per scenario with a leading dimension
 * of their own; 0 shares one vector (or one set of seeds) with every scenario.  pbar_out or
 * q_out must be given; jq_out, info_out and delta_out may be NULL.  Seeds are independent of each
 * other: a non-finite entry of one seed gives non-finite output for that seed only.  The
 * no-gimbal model has nx = 5 and nw = 3N.
 * DEVICE pointers, enqueued on `stream`; never synchronises, and allocates nothing once the
 * handle's workspace covers B (a solve's workspace does).  One wavefront per scenario forms
 * every seed: the factorisation is done once.
 * A NULL handle, B <= 0, na <= 0, a NULL x, p, lam_g, lam_x, lbx, ubx, lbg or ubg, every seed
 * NULL, pbar_out and q_out both NULL, or a leading dimension that is neither 0 nor >= the vector
 * length (nw na, ng na, nx(N+1) na for the seeds) return NMPC_E_INVALID before any device call. */
int nmpc_solve_adjoint_batch_dev(nmpc_handle* h, int32_t B, int32_t na,
                                 const double* x, int64_t ld_x, const double* p, int64_t ld_p,
                                 const double* lam_g, int64_t ld_lam_g, const double* lam_x, int64_t ld_lam_x,
                                 const double* g, int64_t ld_g,
                                 const double* lbx, int64_t ld_lbx, const double* ubx, int64_t ld_ubx,
                                 const double* lbg, int64_t ld_lbg, const double* ubg, int64_t ld_ubg,
                                 const double* x_bar, int64_t ld_x_bar,
                                 const double* lam_g_bar, int64_t ld_lam_g_bar,
                                 const double* X_bar, int64_t ld_X_bar,
                                 double* pbar_out, double* q_out, double* jq_out, int32_t* info_out,
                                 double* delta_out, void* stream);

/* Same with HOST pointers; synchronous (staged through the handle's device buffer). */
int nmpc_solve_adjoint_batch(nmpc_handle* h, int32_t B, int32_t na,
                             const double* x, int64_t ld_x, const double* p, int64_t ld_p,
                             const double* lam_g, int64_t ld_lam_g, const double* lam_x, int64_t ld_lam_x,
                             const double* g, int64_t ld_g,
                             const double* lbx, int64_t ld_lbx, const double* ubx, int64_t ld_ubx,
                             const double* lbg, int64_t ld_lbg, const double* ubg, int64_t ld_ubg,
                             const double* x_bar, int64_t ld_x_bar,
                             const double* lam_g_bar, int64_t ld_lam_g_bar,
                             const double* X_bar, int64_t ld_X_bar,
                             double* pbar_out, double* q_out, double* jq_out, int32_t* info_out,
                             double* delta_out);

/* Forward-mode sensitivity of a SOLUTION, for a whole batch, in one launch: the first-order change
 * of x*, lam_g* and the state trajectory X* with the parameters -- the NMPC law's feedback gain
 * d u0* / d x0 and the prediction x* + (dx* / dp) Dp for a changed initial state or target -- with
 * nothing on the host.  The point (x, lam_g, lam_x, p, g and the four bounds), the barrier weights
 * Sigma_x, Sigma_s, the condensed matrix
 *   M = W + diag(Sigma_x) + delta I + J^T diag(Sigma_s + delta) J
 * and its delta ladder are those of nmpc_solve_adjoint_batch_dev (above); M is factorised once
 * per scenario.  For each of nd >= 1 directions dp_d of the parameters, with the exact parameter
 * derivatives of nmpc_param_products_batch_dev at (x*, lam_g*), obj_factor = 1:
 *   dx_out     (nw nd x B)      : M dx = -(d_p grad_w L) dp_d - J^T Sigma_s (dg/dp) dp_d
 *   dlam_g_out (ng nd x B)      = Sigma_s (J dx + (dg/dp) dp_d): the sum first, then the weight;
 *                                 stage 0's rows, where J is zero, are Sigma_s (dg/dp) dp_d
 *   dX_out     (nx(N+1) nd x B) = (dX/dw) dx + (dX/dp) dp_d, in X_out's layout
 * (dx*, dlam_g*) is the interior-point linearisation of the optimality conditions at the point,
 * and <pbar, dp> = <x_bar, dx> + <lam_g_bar, dlam_g> + <X_bar, dX> holds with the pbar of
 * nmpc_solve_adjoint_batch_dev for every seed.  info_out (B): 0 = factorised with the right
 * inertia; 1 = no rung of the ladder did; -11 = an equality row (lbg == ubg, which needs the
 * augmented system), lbx > ubx, or a weight that is not a finite non-negative number (a NaN
 * multiplier).  With 1 or -11 the scenario's dx, dlam_g and dX are NaN and its neighbours are
 * untouched.  delta_out (B): the delta of the last factorisation tried (0 with -11).
 * g is the row values the weights are taken at (a solve's g_out); NULL = the kernel's own
 * g(x, p).  A variable with lbx == ubx is fixed: it leaves the system and its dx is exactly 0.
 * A direction along an entry of p that nothing reads gives dx, dlam_g and dX equal to 0 (the
 * entry is never loaded: a NaN there changes nothing).  A bound beyond +-1e19 enters the weights'
 * formula as it stands.
 * Within a scenario direction d occupies [d n, (d+1) n) of dp (n = np) and of each output array.
 * x, p, lam_g, lam_x, g and the bounds are n per scenario with a leading dimension of their own;
 * 0 shares one vector with every scenario, and ld_dp = 0 one set of nd directions.  At least one
 * of dx_out, dlam_g_out, dX_out must be given; the others, info_out and delta_out may be NULL.
 * Directions are independent of each other: every per-direction buffer is rewritten by each
 * direction, so a non-finite entry of one direction gives non-finite output for that direction
 * only.  The no-gimbal model has nx = 5 and nw = 3N.
 * DEVICE pointers, enqueued on `stream`; never synchronises, and allocates nothing once the
 * handle's workspace covers B (a solve's workspace does).  One wavefront per scenario forms
 * every direction: the factorisation is done once.
 * A NULL handle, B <= 0, nd <= 0, a NULL x, p, lam_g, lam_x, lbx, ubx, lbg, ubg or dp, every
 * output NULL, or a leading dimension that is neither 0 nor >= the vector length (np nd for dp)
 * return NMPC_E_INVALID before any device call. */
int nmpc_solve_tangent_batch_dev(nmpc_handle* h, int32_t B, int32_t nd,
                                 const double* x, int64_t ld_x, const double* p, int64_t ld_p,
                                 const double* lam_g, int64_t ld_lam_g, const double* lam_x, int64_t ld_lam_x,
                                 const double* g, int64_t ld_g,
                                 const double* lbx, int64_t ld_lbx, const double* ubx, int64_t ld_ubx,
                                 const double* lbg, int64_t ld_lbg, const double* ubg, int64_t ld_ubg,
                                 const double* dp, int64_t ld_dp,
                                 double* dx_out, double* dlam_g_out, double* dX_out, int32_t* info_out,
                                 double* delta_out, void* stream);

/* Same with HOST pointers; synchronous (staged through the handle's device buffer). */
int nmpc_solve_tangent_batch(nmpc_handle* h, int32_t B, int32_t nd,
                             const double* x, int64_t ld_x, const double* p, int64_t ld_p,
                             const double* lam_g, int64_t ld_lam_g, const double* lam_x, int64_t ld_lam_x,
                             const double* g, int64_t ld_g,
                             const double* lbx, int64_t ld_lbx, const double* ubx, int64_t ld_ubx,
                             const double* lbg, int64_t ld_lbg, const double* ubg, int64_t ld_ubg,
                             const double* dp, int64_t ld_dp,
                             double* dx_out, double* dlam_g_out, double* dX_out, int32_t* info_out,
                             double* delta_out);

/* The feedback policy along a SOLUTION's plan, for a whole batch, in one launch: what a controller
 * needs to act between two solves,
 *   u_k(x, p') ~ u*_k + K_k (x - X*_k) + sum_d kff_k^(d) c_d,      p' - p = sum_d c_d dp_d.
 * The point (x, lam_g, lam_x, p, g and the four bounds), the barrier weights, the fixed-variable
 * rule, the validity rules (info = -11), the condensed matrix M and its delta ladder (info = 1),
 * leading dimensions, ld = 0 sharing and the +-1e19 rule are those of nmpc_solve_tangent_batch_dev
 * (above).  With obj_factor = 1 and the stage terms of M's Riccati recursion at the ladder's delta,
 *   R~_k = R_k + B'P_{k+1}B,  S~_k = S_k + B'P_{k+1}A,  K_k = -R~_k^-1 S~_k,  k = N-1 ... 0,
 * where, unlike in every other entry point, stage 0's cross term S_0 = d2_xu (lam_1' T f)' is part
 * of the recursion (Q_0 stays 0): it changes no solve, since K_0 multiplies a zero state step
 * there, and makes K_0 the stage-0 gain.  For each of nd >= 0 directions dp_d, with the
 * right-hand side and xi = (dX/dp) dp_d of nmpc_solve_tangent_batch_dev and the recursion's k_k,
 *   kff_k = k_k - K_k xi_k,
 * so that dx_k = K_k dX_k + kff_k for that entry point's dx and dX, every k = 0 ... N-1.
 * Outputs, per scenario, in the model's own dimensions (the no-gimbal model: nu = 3, nx = 5):
 *   K_out   (nu nx N x B)  : block k is K_k, nu x nx column-major: (i, j) at k nu nx + j nu + i
 *   kff_out (nw nd x B)    : direction d occupies [d nw, (d+1) nw), in dx_out's layout
 *   A_out   (nx nx N x B)  : block k is A_k = d x_{k+1} / d x_k of x_{k+1} = x_k + T f(x_k, u_k)
 *                            at (X*, x*), column-major
 *   B_out   (nx nu N x B)  : block k is B_k = d x_{k+1} / d u_k, nx x nu column-major
 *   X_out   (nx(N+1) x B)  : X*, the kernel's own rollout
 *   info_out, delta_out (B): as nmpc_solve_tangent_batch_dev's
 * Each may be NULL; at least one of K_out, kff_out, A_out, B_out must be given.  With info != 0
 * every output of the scenario is NaN and its neighbours are untouched.  A variable with
 * lbx == ubx is fixed: its row of every K_k and its entry of kff are exactly 0.  nd = 0 is allowed;
 * dp and kff_out must then be NULL.  Directions are independent of each other.
 * DEVICE pointers, enqueued on `stream`; never synchronises, and allocates nothing once the
 * handle's workspace covers B (a solve's workspace does).
 * A NULL handle, B <= 0, nd < 0, a NULL x, p, lam_g, lam_x, lbx, ubx, lbg or ubg, a NULL dp with
 * nd > 0, a dp or kff_out with nd = 0, K_out, kff_out, A_out and B_out all NULL, or a leading
 * dimension that is neither 0 nor >= the vector length (np nd for dp) return NMPC_E_INVALID before
 * any device call. */
int nmpc_solve_policy_batch_dev(nmpc_handle* h, int32_t B, int32_t nd,
                                const double* x, int64_t ld_x, const double* p, int64_t ld_p,
                                const double* lam_g, int64_t ld_lam_g, const double* lam_x, int64_t ld_lam_x,
                                const double* g, int64_t ld_g,
                                const double* lbx, int64_t ld_lbx, const double* ubx, int64_t ld_ubx,
                                const double* lbg, int64_t ld_lbg, const double* ubg, int64_t ld_ubg,
                                const double* dp, int64_t ld_dp,
                                double* K_out, double* kff_out, double* A_out, double* B_out, double* X_out,
                                int32_t* info_out, double* delta_out, void* stream);

/* Same with HOST pointers; synchronous (staged through the handle's device buffer). */
int nmpc_solve_policy_batch(nmpc_handle* h, int32_t B, int32_t nd,
                            const double* x, int64_t ld_x, const double* p, int64_t ld_p,
                            const double* lam_g, int64_t ld_lam_g, const double* lam_x, int64_t ld_lam_x,
                            const double* g, int64_t ld_g,
                            const double* lbx, int64_t ld_lbx, const double* ubx, int64_t ld_ubx,
                            const double* lbg, int64_t ld_lbg, const double* ubg, int64_t ld_ubg,
                            const double* dp, int64_t ld_dp,
                            double* K_out, double* kff_out, double* A_out, double* B_out, double* X_out,
                            int32_t* info_out, double* delta_out);

/* Disturbance rollouts of that policy on the nonlinear plant, for a whole batch, in one launch:
 * what the clamped policy costs and whether it keeps the rows when the state drifts.  For each of B
 * scenarios and each of M samples s, in fp64 and in the model's own dimensions (the no-gimbal model:
 * nu = 3, nx = 5):
 *   x_0 = p[x0 block] + e0[s]
 *   for k = 0 ... N-1:
 *     u_raw = ubar_k + K_k (x_k - Xbar_k)          (K NULL: u_raw = ubar_k, open-loop replay)
 *     u_k   = min(max(u_raw, lbx_k), ubx_k)        (lbx / ubx NULL: that side is not clamped)
 *     J    += stage_cost(x_k; p)                   (summed in stage order)
 *     x_{k+1} = x_k + T f(x_k, u_k) + w_k[s]       (w NULL: no process disturbance)
 *   viol = max over all ng rows r of max(g_r - ubg_r, lbg_r - g_r, 0)
 *          (rows of stages 0 ... N at x_0 ... x_N, g_out's row order; the +-1e19 rule; lbg and
 *          ubg NULL: no row has a bound, viol = 0)
 *   nsat = number of control entries u_k differs from u_raw in
 * The kernel knows nothing about directions: ubar is caller-formed (for a parameter move
 * u* + sum_d kff^(d) c_d, and p the moved parameter vector).  K, Xbar and ubar have the layouts
 * nmpc_solve_policy_batch_dev's K_out and X_out and the solve's x_out have, so those buffers can be
 * passed straight in.  The plant's operations are those of the solve's own rollout in the same
 * order: a sample with e0 = 0, no w and no active clamp reproduces X_out of nmpc_eval_batch_dev.
 * Inputs (leading dimension: 0 shares one column across scenarios, else >= the vector length):
 *   p    (np x B)        required        ubar (nw x B)         required
 *   Xbar (nx(N+1) x B)   required        K    (nu nx N x B)    optional
 *   lbx, ubx (nw x B)    optional, each  lbg, ubg (ng x B)     optional, both or neither
 *   e0   (nx M x B)      required: sample s occupies [s nx, (s+1) nx)
 *   w    (nx N M x B)    optional: sample s, stage k occupy [(s N + k) nx, (s N + k + 1) nx)
 * Outputs, each may be NULL, at least one of J_out, viol_out, X_out, U_out must be given:
 *   J_out, viol_out (M x B), nsat_out (M x B, int32): sample s of scenario b at b M + s
 *   X_out (nx(N+1) x M x B): x_0 ... x_N of sample s of scenario b from (b M + s) nx (N+1)
 *   U_out (nw x M x B)      : u_0 ... u_{N-1} likewise
 * A NaN among a sample's states, controls, row values or the bounds it meets gives NaN in that
 * sample's J and viol only (the row maximum does not drop it); a scenario whose policy is NaN
 * (info != 0) therefore yields NaN samples beside untouched neighbours.  States that leave the
 * cost's domain are reported as they come (inf / NaN), not trapped.
 * DEVICE pointers, enqueued on `stream`; never synchronises, allocates nothing and needs no
 * workspace (each sample's state lives in on-chip memory): the handle's memory is untouched.
 * A NULL handle, B <= 0, M <= 0 (or M > 64 x 65535), a NULL p, ubar, Xbar or e0, J_out, viol_out,
 * X_out and U_out all NULL, lbg without ubg or the reverse, or a leading dimension that is neither
 * 0 nor >= the vector length return NMPC_E_INVALID before any device call. */
int nmpc_policy_rollout_batch_dev(nmpc_handle* h, int32_t B, int32_t M,
                                  const double* p, int64_t ld_p, const double* ubar, int64_t ld_ubar,
                                  const double* Xbar, int64_t ld_Xbar, const double* K, int64_t ld_K,
                                  const double* lbx, int64_t ld_lbx, const double* ubx, int64_t ld_ubx,
                                  const double* lbg, int64_t ld_lbg, const double* ubg, int64_t ld_ubg,
                                  const double* e0, int64_t ld_e0, const double* w, int64_t ld_w,
                                  double* J_out, double* viol_out, int32_t* nsat_out, double* X_out,
                                  double* U_out, void* stream);

/* Same with HOST pointers; synchronous (staged through the handle's device buffer). */
int nmpc_policy_rollout_batch(nmpc_handle* h, int32_t B, int32_t M,
                              const double* p, int64_t ld_p, const double* ubar, int64_t ld_ubar,
                              const double* Xbar, int64_t ld_Xbar, const double* K, int64_t ld_K,
                              const double* lbx, int64_t ld_lbx, const double* ubx, int64_t ld_ubx,
                              const double* lbg, int64_t ld_lbg, const double* ubg, int64_t ld_ubg,
                              const double* e0, int64_t ld_e0, const double* w, int64_t ld_w,
                              double* J_out, double* viol_out, int32_t* nsat_out, double* X_out,
                              double* U_out);

/* The reverse sweep of those rollouts, for a whole batch, in one launch: the gradient of a scalar
 * loss on the sampled costs and trajectories with respect to everything the rollout reads except
 * the bounds.  For scenario b with its M samples, seeds Jb_s on J_s, Xb_s on X_s (nx(N+1)) and Ub_s
 * on the applied controls U_s (nw) define
 *   L_b = sum_s ( Jb_s J_s + <Xb_s, X_s> + <Ub_s, U_s> )
 * with J, X and U as nmpc_policy_rollout_batch_dev defines them.  Like the other adjoint entry
 * points this is a function AT GIVEN TRAJECTORIES: X is the forward call's X_out for the same p,
 * ubar, Xbar, K, lbx and ubx, and is not recomputed.  Per sample, with x_k = X[s, k], backwards:
 *   lam_N = Xb_N
 *   for k = N-1 ... 0:
 *     u_raw = ubar_k + K_k (x_k - Xbar_k),  u_k = clamp(u_raw)      (the forward's operations)
 *     mask_r = 1 where u_k[r] == u_raw[r], else 0     (the forward's nsat rule: u_raw exactly on a
 *                                                      bound counts as unclamped, derivative 1)
 *     A_k = d x_{k+1} / d x_k,  B_k = d x_{k+1} / d u_k   at (x_k, u_k)
 *     mu     = mask . (B_k^T lam_{k+1} + Ub_k)
 *     wbar_k = lam_{k+1}
 *     lam_k  = Jb grad_x l_k(x_k; p) + Xb_k + A_k^T lam_{k+1} + K_k^T mu
 *     ubar_bar_k += mu;   K_bar_k += mu (x_k - Xbar_k)^T;   Xbar_bar_k -= K_k^T mu
 *     p_bar[target x, y] -= Jb (grad_x l_k)[0, 1]   (l depends on position and target through their difference)
 *     p_bar[w1_pidx] += Jb dd_k,  p_bar[w2_pidx] += Jb (Q_k - 1)    (where the index is set: the
 *                       target distance and the field-of-view term; the no-gimbal model has no w2 term)
 *   e0_bar = lam_0;   p_bar[x0 block] += lam_0
 * e0, w and the row bounds are no inputs: given X the sweep does not depend on them.  viol is a
 * maximum and is NOT differentiated; a caller who wants a row penalty seeds Xb with its gradient.
 * The clamp bounds receive no gradient.
 * Inputs (leading dimension: 0 shares one column, or one set of seeds, with every scenario, else >=
 * the vector length):
 *   p    (np x B)          required        ubar (nw x B)          required
 *   Xbar (nx(N+1) x B)     required        K    (nu nx N x B)     optional (NULL: open loop)
 *   lbx, ubx (nw x B)      optional, each
 *   X    (nx(N+1) x M x B) required: the forward call's X_out
 *   Jb   (M x B)           seed            Xb   (nx(N+1) x M x B) seed, X_out's layout
 *   Ub   (nw x M x B)      seed, U_out's layout
 * Each seed may be NULL and then contributes nothing; at least one must be given.
 * Outputs, each may be NULL, at least one of the six double outputs must be given:
 *   ubar_bar_out (nw x B), K_bar_out (nu nx N x B, K_out's layout), Xbar_bar_out (nx(N+1) x B, stage
 *   N exactly 0), p_bar_out (np x B): SUMMED over the scenario's M samples.  An entry of p that J, X
 *   and U do not read (an obstacle centre, the target's third entry, tail entries) is exactly 0
 *   e0_bar_out (nx x M x B, e0's layout), w_bar_out (nx N x M x B, w's layout): per sample
 *   nsat_out (M x B, int32): the clamp count of the recomputed controls; equal to the forward's
 *   nsat when the sweep saw the clamp pattern the forward saw
 * K_bar_out and Xbar_bar_out need K (with K NULL nothing depends on them).
 * The sums over samples are sums in a FIXED order: within a block of 64 samples the order depends
 * on the sample numbers alone, never on the data, and the blocks are added in ascending order; no
 * floating-point atomics are used, so two identical calls agree bitwise, and the result at M > 64
 * is fl(sum over samples 0 ... 63 + sum over samples 64 ... 127 + ...).  Being a sum, a reduced
 * output takes a NaN from any one sample: a NaN in a sample's X, seeds, controls or the bounds it
 * meets makes that sample's e0_bar and w_bar NaN and every entry of its own scenario's reduced
 * outputs that the rollout reads NaN; other scenarios are untouched.
 * DEVICE pointers, enqueued on `stream`; never synchronises.  With M <= 64 it needs no workspace
 * and leaves the handle's memory untouched; with M > 64 the per-block partial sums (ceil(M / 64) x
 * (nw + nu nx N + nx (N+1) + np) doubles per scenario) go to the handle's workspace, grown only when
 * it does not cover them yet.
 * A NULL handle, B <= 0, M <= 0 (or M > 64 x 65535), a NULL p, ubar, Xbar or X, Jb, Xb and Ub all
 * NULL, the six double outputs all NULL, K_bar_out or Xbar_bar_out with a NULL K, or a leading
 * dimension that is neither 0 nor >= the vector length return NMPC_E_INVALID before any device call. */
int nmpc_policy_rollout_adjoint_batch_dev(nmpc_handle* h, int32_t B, int32_t M,
                                          const double* p, int64_t ld_p, const double* ubar, int64_t ld_ubar,
                                          const double* Xbar, int64_t ld_Xbar, const double* K, int64_t ld_K,
                                          const double* lbx, int64_t ld_lbx, const double* ubx, int64_t ld_ubx,
                                          const double* X, int64_t ld_X, const double* Jb, int64_t ld_Jb,
                                          const double* Xb, int64_t ld_Xb, const double* Ub, int64_t ld_Ub,
                                          double* ubar_bar_out, double* K_bar_out, double* Xbar_bar_out,
                                          double* p_bar_out, double* e0_bar_out, double* w_bar_out,
                                          int32_t* nsat_out, void* stream);

/* Same with HOST pointers; synchronous (staged through the handle's device buffer). */
int nmpc_policy_rollout_adjoint_batch(nmpc_handle* h, int32_t B, int32_t M,
                                      const double* p, int64_t ld_p, const double* ubar, int64_t ld_ubar,
                                      const double* Xbar, int64_t ld_Xbar, const double* K, int64_t ld_K,
                                      const double* lbx, int64_t ld_lbx, const double* ubx, int64_t ld_ubx,
                                      const double* X, int64_t ld_X, const double* Jb, int64_t ld_Jb,
                                      const double* Xb, int64_t ld_Xb, const double* Ub, int64_t ld_Ub,
                                      double* ubar_bar_out, double* K_bar_out, double* Xbar_bar_out,
                                      double* p_bar_out, double* e0_bar_out, double* w_bar_out,
                                      int32_t* nsat_out);

/* The closed-loop covariance of that policy around the plan, for a whole batch, in one launch: the
 * number the rollouts only estimate, and from it the standard deviation of every row and every
 * control -- what a stochastic-NMPC user tightens lbg / ubg / lbx / ubx by before the next solve
 * (the "back-offs").  For each of B scenarios and each of nc >= 1 covariance cases c, in fp64 and in
 * the model's own dimensions (the no-gimbal model: nu = 3, nx = 5), to first order around the plan:
 *   Sigma_0 = S0[c]
 *   for k = 0 ... N-1:
 *     A_k, B_k   = d x_{k+1} / d x_k, d x_{k+1} / d u_k of x_{k+1} = x_k + T f(x_k, u_k) at
 *                  (Xbar_k, ubar_k): A_out, B_out of nmpc_solve_policy_batch_dev
 *     Acl_k      = A_k + B_k K_k                        (K NULL: Acl_k = A_k, open loop)
 *     var_u[k,r] = (K_k Sigma_k K_k^T)[r,r]             (K NULL: 0)
 *     var_g[k,i] = Sigma_k[bi,bi]                       box row i on state bi
 *                = g^T Sigma_k[0:2,0:2] g + obs_var[o]  obstacle row o, g = -(x - ox, y - oy) / d at
 *                                                       Xbar_k, the centre taken from p where the
 *                                                       descriptor says so
 *     Sigma_{k+1} = Acl_k Sigma_k Acl_k^T + W[c]        (W NULL: no process noise)
 *   var_g[N, .] at Sigma_N, Xbar_N
 *   sigma = sqrt(max(var, 0)); a NaN variance gives NaN (the maximum does not drop it)
 * The kernel knows nothing about clamps: a control held on its bound passes no feedback, and a
 * caller who wants that zeroes the control's row of K_k.  W is the same at every stage.
 * p, ubar, Xbar and K are nmpc_policy_rollout_batch_dev's, so K_out and X_out of
 * nmpc_solve_policy_batch_dev and the solve's x_out can be passed straight in.
 * Inputs (leading dimension: 0 shares one column across scenarios, else >= the vector length):
 *   p       (np x B)         required: read only for obstacle centres taken from p
 *   ubar    (nw x B)         required        Xbar (nx(N+1) x B)   required
 *   K       (nu nx N x B)    optional, K_out's layout
 *   S0      (nx nx nc x B)   required: case c occupies [c nx nx, (c+1) nx nx), column-major
 *   W       (nx nx nc x B)   optional, as S0
 *   obs_var (n_obs x B)      optional: the isotropic variance of each obstacle's centre, shared by
 *                            the cases
 * Only the lower triangle (i >= j) of each S0 and W block is read; the upper one is taken as its mirror.
 * Outputs, each may be NULL, at least one must be given; case c of scenario b starts at (b nc + c) n:
 *   Sigma_out   (nx nx (N+1) x nc x B): block k is Sigma_k, column-major, exactly symmetric
 *   sigma_u_out (nw x nc x B)         : x_out's layout
 *   sigma_g_out (ng x nc x B)         : g_out's row order; stage 0's rows are taken at Sigma_0
 * Cases are independent: a NaN in one case's S0 or W stays in that case.  A NaN K or Xbar (a policy
 * with info != 0) makes that scenario's Sigma_k (k >= 1) and sigma_u NaN beside untouched
 * neighbours.  S0 = 0 with W NULL gives exactly 0 everywhere.
 * DEVICE pointers, enqueued on `stream`; never synchronises, allocates nothing and needs no
 * workspace (each case's matrices live in on-chip memory): the handle's memory is untouched.
 * A NULL handle, B <= 0, nc <= 0 (or nc > 65535), a NULL p, ubar, Xbar or S0, Sigma_out, sigma_u_out
 * and sigma_g_out all NULL, obs_var on a problem with n_obs = 0, or a leading dimension that is
 * neither 0 nor >= the vector length return NMPC_E_INVALID before any device call. */
int nmpc_policy_covariance_batch_dev(nmpc_handle* h, int32_t B, int32_t nc,
                                     const double* p, int64_t ld_p, const double* ubar, int64_t ld_ubar,
                                     const double* Xbar, int64_t ld_Xbar, const double* K, int64_t ld_K,
                                     const double* S0, int64_t ld_S0, const double* W, int64_t ld_W,
                                     const double* obs_var, int64_t ld_obs_var,
                                     double* Sigma_out, double* sigma_u_out, double* sigma_g_out, void* stream);

/* Same with HOST pointers; synchronous (staged through the handle's device buffer). */
int nmpc_policy_covariance_batch(nmpc_handle* h, int32_t B, int32_t nc,
                                 const double* p, int64_t ld_p, const double* ubar, int64_t ld_ubar,
                                 const double* Xbar, int64_t ld_Xbar, const double* K, int64_t ld_K,
                                 const double* S0, int64_t ld_S0, const double* W, int64_t ld_W,
                                 const double* obs_var, int64_t ld_obs_var,
                                 double* Sigma_out, double* sigma_u_out, double* sigma_g_out);

/* The reverse sweep of that covariance, for a whole batch, in one launch: the gradient of a loss on
 * the covariances and the back-offs with respect to everything the forward call reads -- the gains,
 * the noise model, the plan and p -- so the chain solve -> policy -> covariance -> tighten -> next solve
 * can be differentiated.  For each of B scenarios and each of nc cases, at the Sigma_k the forward call
 * returned (Sigma_out; an input here, not recomputed), with seeds Sb_k on Sigma_k (k = 0 ... N), ub on
 * the VARIANCES var_u = sigma_u^2 and gb on var_g = sigma_g^2 (the square root's chain rule is the
 * caller's: var_bar = sigma_bar / (2 sigma)), the gradient of
 *   L = sum_k <Sb_k, Sigma_k> + <ub, var_u> + <gb, var_g>
 * by the recursion, with sym(S) = (S + S^T) / 2 and Lam symmetric throughout,
 *   R_k(Lam): Lam[bi,bi] += gb[k,i]                      box row i on state bi
 *             Lam[0:2,0:2] += gb[k,o] g g^T              obstacle row o, g as in the forward call
 *             obs_var_bar[o] += gb[k,o]
 *             pos = H_o (2 gb[k,o] Sigma_k[0:2,0:2] g)   H_o: the row's Hessian in (x, y) at Xbar_k
 *             Xbar_bar[k,0:2] += pos;  p_bar[centre of o, where taken from p] -= pos
 *   Lam_N = sym(Sb_N) + R_N
 *   for k = N-1 ... 0:
 *     M = Lam_{k+1} Acl_k,   G = 2 M Sigma_k
 *     K_bar_k = B_k^T G + 2 diag(ub_k) K_k Sigma_k
 *     (Xbar_bar_k, ubar_bar_k) += <G, dA_k> + <G K_k^T, dB_k> pulled back through the entries of A_k and
 *                                 B_k, which depend on theta, psi (Xbar_k[3], [4]) and v (ubar_k[0]) alone
 *     Lam_k = Acl_k^T M + sym(Sb_k) + K_k^T diag(ub_k) K_k + R_k
 *   S0_bar = Lam_0,   W_bar = Lam_N + Lam_{N-1} + ... + Lam_1 (added in that order)
 * Lam_k is the gradient with respect to a covariance injected at stage k: what a stage-varying W needs.
 * With K NULL, Acl_k = A_k, var_u_bar contributes nothing and K_bar_out must be NULL.  Neither the clamp
 * nor the bounds are inputs.
 * Inputs (leading dimension: 0 shares one column across scenarios, else >= the vector length):
 *   p, ubar, Xbar, K                  the forward call's, p, ubar and Xbar required
 *   Sigma     (nx nx (N+1) nc x B)    required: the forward call's Sigma_out; only the lower triangle
 *                                     (i >= j) of each block is read
 *   Sigma_bar (nx nx (N+1) nc x B)    optional seed, Sigma's layout; any nx x nx blocks, symmetrised here
 *   var_u_bar (nw nc x B)             optional seed, sigma_u_out's layout
 *   var_g_bar (ng nc x B)             optional seed, sigma_g_out's layout
 * At least one seed must be given.
 * Outputs, each may be NULL, at least one must be given; case c of scenario b starts at (b nc + c) n,
 * and a caller whose input is shared by the cases or the scenarios sums:
 *   S0_bar_out      (nx nx x nc x B)        exactly symmetric: the G with dL = sum_ij G_ij dS_ij for
 *                                           symmetric dS
 *   W_bar_out       (nx nx x nc x B)        likewise
 *   Lambda_out      (nx nx (N+1) x nc x B)  block k is Lam_k; block 0 equals S0_bar_out bitwise
 *   obs_var_bar_out (n_obs x nc x B)
 *   K_bar_out       (nu nx N x nc x B)      K_out's layout; needs K
 *   ubar_bar_out    (nw x nc x B)
 *   Xbar_bar_out    (nx(N+1) x nc x B)
 *   p_bar_out       (np x nc x B)           exactly 0 outside the obstacle centres taken from p; obstacles
 *                                           that name one entry are added in ascending order
 * No floating-point atomics: two identical calls agree bitwise.  Cases are independent: a NaN in one
 * case's Sigma or seeds stays in that case, a NaN K or plan of one scenario leaves its neighbours
 * untouched.  All seeds 0 with finite inputs give exactly 0 everywhere.
 * DEVICE pointers, enqueued on `stream`; never synchronises, allocates nothing and needs no
 * workspace: the handle's memory is untouched.
 * Return NMPC_E_INVALID before any device call, in this order: a NULL handle; B <= 0; nc <= 0 (or
 * nc > 65535); a NULL p, ubar, Xbar or Sigma; every seed NULL; every output NULL; K_bar_out with a NULL
 * K; obs_var_bar_out on a problem with n_obs = 0; a leading dimension that is neither 0 nor >= the
 * vector length. */
int nmpc_policy_covariance_adjoint_batch_dev(nmpc_handle* h, int32_t B, int32_t nc,
                                             const double* p, int64_t ld_p, const double* ubar, int64_t ld_ubar,
                                             const double* Xbar, int64_t ld_Xbar, const double* K, int64_t ld_K,
                                             const double* Sigma, int64_t ld_Sigma,
                                             const double* Sigma_bar, int64_t ld_Sigma_bar,
                                             const double* var_u_bar, int64_t ld_var_u_bar,
                                             const double* var_g_bar, int64_t ld_var_g_bar,
                                             double* S0_bar_out, double* W_bar_out, double* Lambda_out,
                                             double* obs_var_bar_out, double* K_bar_out, double* ubar_bar_out,
                                             double* Xbar_bar_out, double* p_bar_out, void* stream);

/* Same with HOST pointers; synchronous (staged through the handle's device buffer). */
int nmpc_policy_covariance_adjoint_batch(nmpc_handle* h, int32_t B, int32_t nc,
                                         const double* p, int64_t ld_p, const double* ubar, int64_t ld_ubar,
                                         const double* Xbar, int64_t ld_Xbar, const double* K, int64_t ld_K,
                                         const double* Sigma, int64_t ld_Sigma,
                                         const double* Sigma_bar, int64_t ld_Sigma_bar,
                                         const double* var_u_bar, int64_t ld_var_u_bar,
                                         const double* var_g_bar, int64_t ld_var_g_bar,
                                         double* S0_bar_out, double* W_bar_out, double* Lambda_out,
                                         double* obs_var_bar_out, double* K_bar_out, double* ubar_bar_out,
                                         double* Xbar_bar_out, double* p_bar_out);

/* The cost-to-go expansion of that policy, for a whole batch, in one launch: the expected cost of the
 * closed loop under an uncertain initial state and process noise, exact to second order -- the number
 * the mean of the rollouts' sampled J estimates with O(1 / sqrt(M)) noise -- its variance to first
 * order, and a local quadratic model of the cost-to-go at every stage.  For each of B scenarios, in
 * fp64 and in the model's own dimensions (the no-gimbal model: nu = 3, nx = 5), at the GIVEN plan
 * (Xbar_k, ubar_k), k = 0 ... N, and gains K_k:
 *   the policy is u_k = ubar_k + K_k (x_k - Xbar_k), UNCLAMPED (K NULL: K_k = 0, open loop);
 *   the plant is  x_{k+1} = x_k + T f(x_k, u_k) + w_k, started from x_0 + e0, e0 ~ (0, S0), w_k ~ (0, W);
 *   the cost is   J = sum_{k < N} l_k(x_k; p), the stage cost as the rollouts sum it: it reads the state
 *                 only, and stage N carries no cost.
 * With V_k(x) the cost from stage k on without noise, lam_k = grad V_k and P_k = grad^2 V_k at Xbar_k:
 *   lam_N = 0,  P_N = 0
 *   for k = N-1 ... 0:
 *     g_k, H_k = gradient and Hessian of l_k at Xbar_k
 *     A_k, B_k = d x_{k+1} / d x_k, d x_{k+1} / d u_k at (Xbar_k, ubar_k);  Acl_k = A_k + B_k K_k, each
 *                entry fl(A + fl(B K)) as nmpc_policy_covariance_batch_dev rounds it
 *     Fxx, Fxu = second derivatives of lam_{k+1}^T T f at (Xbar_k, ubar_k): the dynamics' curvature
 *                shifts the mean at the same order as the cost's (entries (theta, psi) x (theta, psi)
 *                and (theta, psi) x speed only)
 *     M_k   = H_k + Fxx + Fxu K_k + K_k^T Fxu^T       (the policy is affine: no further term)
 *     lam_k = g_k + Acl_k^T lam_{k+1}
 *     P_k   = M_k + Acl_k^T P_{k+1} Acl_k
 *   J       = sum_k l_k(Xbar_k)
 *   per case c, with <P, S> = sum_i P_ii S_ii + 2 sum_{i > j} P_ij S_ij:
 *   dJ[c]   = 1/2 <P_0, S0[c]> + 1/2 <P_N + ... + P_1, W[c]>          E[J] = J + dJ to second order
 *   varJ[c] = lam_0^T S0[c] lam_0 + sum_{k >= 1} lam_k^T W[c] lam_k   Var[J] to first order
 * P_k may be indefinite: that is the model, and nothing is done about it.  W is the same at every
 * stage, so its terms are summed over the stages before the cases.  The expansion is at the points
 * given; it is the closed loop's own undisturbed trajectory -- and J + dJ the expected cost -- when Xbar
 * is the plant's rollout of ubar from p's initial state, which X_out of nmpc_solve_policy_batch_dev
 * with the solve's x_out is.  Neither the clamp, nor the rows, nor the bounds are inputs.
 * Inputs: p, ubar, Xbar, K, S0 and W are nmpc_policy_covariance_batch_dev's, with its layouts and its
 * leading-dimension rule (0 shares one column across scenarios, else >= the vector length); p, ubar and
 * Xbar are required, K optional.  nc >= 0: with nc = 0 there are no cases and S0, W, dJ_out and varJ_out
 * must be NULL; with nc > 0 S0 is required and W NULL means no process noise.  Only the lower triangle
 * (i >= j) of each S0 and W block is read.
 * Outputs, each may be NULL, at least one must be given:
 *   J_out    (B)
 *   lam_out  (nx(N+1) x B)       : X_out's layout; block N is exactly 0
 *   P_out    (nx nx (N+1) x B)   : block k is P_k, column-major, exactly symmetric; block N is exactly 0
 *   dJ_out   (nc x B)            varJ_out (nc x B)
 * Cases are independent: a NaN in one case's S0 or W stays in that case's dJ and varJ.  A NaN K or Xbar
 * (a policy with info != 0) makes that scenario's J, lam_0, P_0, dJ and varJ NaN beside bitwise-untouched
 * neighbours (J is set to NaN where lam_0 holds one).  S0 = 0 with W NULL gives dJ = varJ = 0.  With
 * N = 1, P_0 = H_0 exactly and K has no effect.  No floating-point atomics: two identical calls agree
 * bitwise.
 * DEVICE pointers, enqueued on `stream`; never synchronises.  Workspace: one slice of
 * nmpc_products_batch_dev's per scenario (the controls, the stage costs' gradients and Hessians, the
 * transcendental cache and the row scaling: 68 doubles for each of 64 stages, 34,816 bytes), taken from the handle's workspace, which is
 * grown only when it does not cover B yet (a solve's workspace does); nothing else is allocated.
 * Return NMPC_E_INVALID before any device call, in this order: a NULL handle; B <= 0; nc < 0; a NULL
 * p, ubar or Xbar; a NULL S0 with nc > 0; S0, W, dJ_out or varJ_out given with nc = 0; every output
 * NULL; a leading dimension that is neither 0 nor >= the vector length. */
int nmpc_policy_value_batch_dev(nmpc_handle* h, int32_t B, int32_t nc,
                                const double* p, int64_t ld_p, const double* ubar, int64_t ld_ubar,
                                const double* Xbar, int64_t ld_Xbar, const double* K, int64_t ld_K,
                                const double* S0, int64_t ld_S0, const double* W, int64_t ld_W,
                                double* J_out, double* lam_out, double* P_out, double* dJ_out,
                                double* varJ_out, void* stream);

/* Same with HOST pointers; synchronous (staged through the handle's device buffer). */
int nmpc_policy_value_batch(nmpc_handle* h, int32_t B, int32_t nc,
                            const double* p, int64_t ld_p, const double* ubar, int64_t ld_ubar,
                            const double* Xbar, int64_t ld_Xbar, const double* K, int64_t ld_K,
                            const double* S0, int64_t ld_S0, const double* W, int64_t ld_W,
                            double* J_out, double* lam_out, double* P_out, double* dJ_out, double* varJ_out);

/* Optional per-iteration trace (debugging / parity): when enabled, the next
 * solve records NMPC_TRACE_FIELDS doubles per iteration per scenario into a
 * device buffer readable with nmpc_read_trace (host pointer,
 * B x (max_iter+3) x NMPC_TRACE_FIELDS, row-major; the last two rows of each
 * scenario are reserved for diagnostic phase timers).  Row i (0 <= i <= max_iter) holds
 *   [0..7]  {iter, mu, f_scaled, theta, delta_w, alpha_pr, alpha_du, ls_trials}
 *           after iteration i+1 (ls_trials < 0: a restoration iteration; i < max_iter), and
 *   [8..11] the convergence check at iteration count i:
 *           {scaled NLP error, dual infeasibility / s_d, constraint violation,
 *            complementarity / s_c} (IpoptCalculatedQuantities::curr_nlp_error); a
 *           NEGATIVE (sign bit set) error marks the restoration NLP's own check
 *           (RestoIpoptNLP), which replaces the main check recorded at the same count. */
#define NMPC_TRACE_FIELDS 12
int nmpc_set_trace(nmpc_handle* h, int32_t enable);
int nmpc_read_trace(nmpc_handle* h, int32_t B, double* host_out);

/* Closed-loop shift (the caller side of the solve, Python/NMPC_TT.py:13-30),
 * on DEVICE pointers, enqueued on `stream`: for each scenario, x0 <- x0 + T f(x0,u0),
 * warm start u <- [u(:,2:N), u(:,N)], target xs <- xs + T [v cos, v sin, w].
 * p (np x B, ld_p) is updated in place (x0 = p[0:8], xs = p[8:11]); w_out
 * (nw x B) receives the shifted warm start; v_t, w_t (length B) are the target
 * speeds (Python/NMPC_TT.py:25).  No-gimbal model: x0 = p[0:5], xs = p[5:8],
 * 3 controls per stage (MATLAB/Dynamic Obstacles/shift1.m). */
int nmpc_shift_dev(nmpc_handle* h, int32_t B, double* p, int64_t ld_p,
                   const double* u_sol, double* w_out,
                   const double* v_t, const double* w_t, void* stream);

/* K closed-loop MPC steps for each of B scenarios in ONE device launch: the
 * reference's main loop (Python/NMPC_TT.py:348-402: solve at :358-365, then
 * shift_timestep at :382 / :13-30) with each scenario advancing on its own
 * wavefront, so no step waits for another scenario's slowest solve.  Step k
 * solves with x0 = w (warm start) and p, records x0 = p[0:8] (x_hist), the
 * applied control u0 = x[0:6] (u_hist), f, status and iterations, then applies
 * x0 <- x0 + T f(x0,u0), w <- [u(:,2:N), u(:,N)], xs <- xs + T [v cos, v sin, w]
 * with the target controls (v, w) = (v_t, w_t)[k*ld_tk + b*ld_tb] (the
 * scripts' con_t schedules: ld_tk = 1, ld_tb = 0 for one shared schedule;
 * ld_tk = 0 for constant controls), and records the FOV-centre error
 * |FOV(x0_{k+1}) - xs_k[0:2]| (Python/NMPC_TT.py:397-400,433-437) in fov_hist.
 * p_step (nullable, K x np with leading dimension ld_ps, shared by all
 * scenarios) is added to p[11:np] after step k: moving obstacles, e.g. the
 * +-1 m/step windows of MATLAB/Dynamic Obstacles/Dynamic Obstacle avoidance.m:213-230.
 * DEVICE pointers, enqueued on `stream`.
 *   p   : np x B (ld_p >= np), in/out (advanced K steps)
 *   w   : nw x B (ld nw), in: first warm start; out: the last step's shifted solution
 *   No-gimbal model: the same loop on [x0(5); xs(3)] and 3 controls per stage
 *   (MATLAB/Dynamic Obstacles/NMPC_TT.m:150-183, shift1.m); histories keep the
 *   widths below with absent gimbal entries 0, and the FOV centre of a camera
 *   without gimbal angles is the UAV's ground position (x, y).
 *   u_hist K x B x 6, x_hist K x B x 8, f_hist / fov_hist / status_hist /
 *   iters_hist K x B; each nullable.  Bounds as in nmpc_solve_batch_dev.
 *   order: nullable, B int32 (device): a permutation of 0..B-1 giving the order in
 *          which scenarios are dispatched to wavefronts (order[g] runs g-th).  Results
 *          do not depend on it.  Putting the longest expected chains first (e.g.
 *          sorted by the previous launch's iterations, nmpc_amd.schedule) keeps a
 *          long chain from starting after the first wave of slots has drained.
 *          Entries outside [0,B) are skipped; a duplicated or missing scenario leaves
 *          some scenario short of its K steps, which nmpc_closed_loop_info reports. */
int nmpc_closed_loop_dev(nmpc_handle* h, int32_t B, int32_t K,
                         const double* lbx, int64_t ld_lbx, const double* ubx, int64_t ld_ubx,
                         const double* lbg, int64_t ld_lbg, const double* ubg, int64_t ld_ubg,
                         double* p, int64_t ld_p, double* w,
                         const double* v_t, const double* w_t, int64_t ld_tk, int64_t ld_tb,
                         const double* p_step, int64_t ld_ps,
                         double* u_hist, double* x_hist, double* f_hist, double* fov_hist,
                         int32_t* status_hist, int32_t* iters_hist, const int32_t* order, void* stream);

/* Scheduling of the last nmpc_closed_loop_dev launch (any pointer may be NULL).  When
 * sched_err or steps_done is requested it first synchronises the stream that launch
 * was enqueued on (hipStreamSynchronize), so it is valid for non-blocking streams.
 *   policy: 0 = one workgroup per scenario running its K steps back to back (B <=
 *     resident waves, a device without exactly 8 XCDs, or NMPC_CLOSED_LOOP=static);
 *     1 = step queues: persistent waves claim (scenario, step) pairs whose previous step
 *     is done, lowest step first, each scenario pinned to one XCD.
 *   resident: waves the closed-loop kernel keeps resident (occupancy x CUs; 0 before
 *     the first launch).  waves: workgroups the last launch started.
 *   sched_err: bit 0 a wave gave up waiting for a published step, bit 1 a scenario did
 *     not complete its K steps (its unrun steps carry status and iterations
 *     NMPC_STATUS_NOT_RUN and NaN f / fov / u / x in the histories), bit 2 the batch has
 *     equality rows and the equality workspace was not reserved (nmpc_reserve_eq): no step
 *     ran, and they carry NMPC_STATUS_EQ_UNRESERVED instead.  0 on success.
 *   steps_done: closed-loop steps completed, counted per scenario by a check kernel
 *     after either policy's launch (must equal B*K; 64-bit). */
#define NMPC_STATUS_NOT_RUN (-1000)
int nmpc_closed_loop_info(nmpc_handle* h, int32_t* policy, int32_t* resident, int32_t* sched_err,
                          int32_t* waves, int64_t* steps_done);

const char* nmpc_last_error(void);

/* Diagnostics: with NMPC_STEP_TIMES set in the environment, nmpc_closed_loop_dev records
 * for every (step k, scenario b) the s_memrealtime stamps (100 MHz) at the start and end
 * of the step and the running wave with the step's shader-clock cycles (s_memtime):
 * XCC_ID | workgroup << 8 | cycles << 24, K x B x 3 uint64; this
 * copies the last launch's record to host_out (n >= 3 K B). */
int nmpc_closed_loop_times(nmpc_handle* h, uint64_t* host_out, int64_t n);

/* Hash of the source, header and compile flags the library was built from
 * (__graft_entry__.source_hash); tests compare it with the checked-out source. */
const char* nmpc_build_id(void);

/* Launch geometry / workspace of the last solve, for measurement. */
int nmpc_kernel_info(const nmpc_handle* h, int32_t* lds_bytes, int32_t* threads_per_scenario);

/* Device workspace the handle holds (bytes): the problem class's per-scenario
 * workspace, and the equality class's, which is allocated only by
 * nmpc_reserve_eq or by a host-pointer batch with equality rows (lbg == ubg) and is 0 until
 * then; per scenario: the class layouts' sizes (ws_per_scenario, wsE_per_scenario; nullable). */
int nmpc_memory_info(const nmpc_handle* h, int64_t* ws_bytes, int64_t* ws_eq_bytes, int64_t* ws_per_scenario,
                     int64_t* wsE_per_scenario);

#ifdef __cplusplus
}
#endif
#endif /* NMPC_AMD_H */
