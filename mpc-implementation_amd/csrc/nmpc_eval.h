// nmpc_eval.h -- what the host translation unit (the C-ABI in nmpc_solve.hip) and the
// evaluation kernel's translation unit (nmpc_eval.hip) share: the kernel's argument block,
// its slice of the handle's per-scenario workspace, and the launcher.  Included by both after
// nmpc_impl::Params is defined; none of the solver's class translation units sees it.
#ifndef NMPC_EVAL_H
#define NMPC_EVAL_H

namespace nmpc_impl {

// DEVICE pointers, layouts and leading dimensions as nmpc_eval_batch_dev (include/nmpc_amd.h);
// x and p are required, every other pointer may be null
struct EvalIO {
  const double *x, *p, *lam_g, *lam_x, *lbx, *ubx, *lbg, *ubg;
  long long ld_x, ld_p, ld_lam_g, ld_lam_x, ld_lbx, ld_ubx, ld_lbg, ld_ubg;
  double *f, *g, *X, *grad_f, *grad_l, *kkt;
  double* ws;  // B x kEvalWs doubles of the handle's workspace
};

// Per-scenario workspace (doubles), sized for N = NMPC_MAX_N and 5 + NMPC_MAX_OBS rows per
// stage: the controls in the kernel's 6-per-stage layout, the stage-cost gradients, the
// transcendental cache of the rollout and stage costs (12 per stage) and the row scaling
// (ones) the solver's adjoint multiplies by.  Every solver class's own workspace is larger
// (static_assert in nmpc_eval.hip), so a handle whose workspace covers B for a solve covers
// B for an evaluation.
constexpr int kEvalStages = NMPC_MAX_N + 1;
constexpr int kEvalU = 0;
constexpr int kEvalGl = kEvalU + 6 * kEvalStages;
constexpr int kEvalTc = kEvalGl + 8 * kEvalStages;
constexpr int kEvalDc = kEvalTc + 12 * kEvalStages;
constexpr int kEvalWs = kEvalDc + (5 + NMPC_MAX_OBS) * kEvalStages;

// DEVICE pointers, layouts and leading dimensions as nmpc_products_batch_dev
// (include/nmpc_amd.h); x, p and v are required, lam_g and every output may be null
struct ProdIO {
  const double *x, *p, *lam_g, *v;
  long long ld_x, ld_p, ld_lam_g, ld_v;
  double obj_factor;
  int nv;
  double *jv, *hv, *dX;
  double* ws;  // B x chunks x kProdWs doubles of the handle's workspace
};

// Per-wavefront workspace of the products kernel (nmpc_products.hip): the evaluation's
// slices plus the stage-cost Hessians (21 per stage).  The stage-cost gradients' slice is
// reused per direction for h_k = Hxx_k dX_k + Hxu_k du_k once the dynamics multipliers are
// formed.  A scenario's directions may be dealt to several wavefronts (chunks), each with a
// slice of its own; every solver class's workspace holds at least one (static_assert in
// nmpc_products.hip), and the host never picks more chunks than the class's workspace covers.
constexpr int kProdU = 0;
constexpr int kProdGl = kProdU + 6 * kEvalStages;
constexpr int kProdHl = kProdGl + 8 * kEvalStages;
constexpr int kProdTc = kProdHl + 21 * kEvalStages;
constexpr int kProdDc = kProdTc + 12 * kEvalStages;
constexpr int kProdWs = kProdDc + (5 + NMPC_MAX_OBS) * kEvalStages;
constexpr int kProdMaxChunks = 16;
// wavefronts a launch is brought up to by chunking: one per SIMD of the MI355X's 256 CUs.
// Measured with 8 directions at the config-3 shape: B = 256 gains 1.7x from 4
// wavefronts per scenario, B = 1,024 and 4,096 lose 10 to 30 % with more than one.
constexpr long long kProdFillWaves = 1024;

// DEVICE pointers, layouts and leading dimensions as nmpc_kkt_solve_batch_dev
// (include/nmpc_amd.h); x and p are required, one of r_w / r_g and one of dw / dX / jdw
struct KktIO {
  const double *x, *p, *lam_g, *sigma_x, *sigma_s, *delta, *r_w, *r_g;
  long long ld_x, ld_p, ld_lam_g, ld_sigma_x, ld_sigma_s, ld_delta, ld_r_w, ld_r_g;
  double obj_factor;
  int nr;
  double *dw, *dX, *jdw;
  int* info;
  double* ws;  // B x kKktWs doubles of the handle's workspace
};

// Per-scenario workspace of the KKT kernel (nmpc_kkt.hip): the products kernel's slices, the
// stage summaries Q_k (36 per stage), the Riccati factors K_k (48), R~_k (21) and k_k (6),
// sigma_x in the kernel's 6-per-stage layout, and one right-hand side's control terms and
// step.  Sized for N = NMPC_MAX_N like the slices above; every solver class's workspace is
// larger (static_assert in nmpc_kkt.hip), so a handle whose workspace covers B for a solve
// covers B here.
constexpr int kKktU = 0;
constexpr int kKktGl = kKktU + 6 * kEvalStages;
constexpr int kKktHl = kKktGl + 8 * kEvalStages;
constexpr int kKktTc = kKktHl + 21 * kEvalStages;
constexpr int kKktDc = kKktTc + 12 * kEvalStages;
constexpr int kKktQs = kKktDc + (5 + NMPC_MAX_OBS) * kEvalStages;
constexpr int kKktK = kKktQs + 36 * kEvalStages;
constexpr int kKktRk = kKktK + 48 * kEvalStages;
constexpr int kKktKf = kKktRk + 21 * kEvalStages;
constexpr int kKktRd = kKktKf + 6 * kEvalStages;
constexpr int kKktRv = kKktRd + 6 * kEvalStages;
constexpr int kKktDu = kKktRv + 6 * kEvalStages;
constexpr int kKktWs = kKktDu + 6 * kEvalStages;

// DEVICE pointers, layouts and leading dimensions as nmpc_param_products_batch_dev
// (include/nmpc_amd.h); x and p are required, dp with nd > 0, lam_g and every output may be null
struct PprodIO {
  const double *x, *p, *lam_g, *dp;
  long long ld_x, ld_p, ld_lam_g, ld_dp;
  double obj_factor;
  int nd;
  double *jp, *hp, *dXp, *gp;
  double* ws;  // B x chunks x kPprodWs doubles of the handle's workspace
};

// Per-wavefront workspace of the parameter-products kernel (nmpc_pproducts.hip): the products
// kernel's slices plus, per stage and obstacle, the three entries of lam_{k,o} grad^2 g_o (an
// obstacle whose centre comes from p moves against the state, each by its own amount, so its
// curvature cannot be summed into the stage's once for all directions).  Chunks as the
// products kernel's; every solver class's workspace holds at least one slice (static_assert
// in nmpc_pproducts.hip).
constexpr int kPprodOc = kProdWs;
constexpr int kPprodWs = kPprodOc + 3 * NMPC_MAX_OBS * kEvalStages;

// DEVICE pointers, layouts and leading dimensions as nmpc_adjoint_products_batch_dev
// (include/nmpc_amd.h); x and p are required, one of the seeds y / z / Xb and one of wbar / pbar
struct AdjIO {
  const double *x, *p, *lam_g, *y, *z, *Xb;
  long long ld_x, ld_p, ld_lam_g, ld_y, ld_z, ld_Xb;
  double obj_factor;
  int na;
  double *wbar, *pbar;
  double* ws;  // B x chunks x kAdjWs doubles of the handle's workspace
};

// Per-wavefront workspace of the adjoint-products kernel (nmpc_adjoint.hip): the
// parameter-products kernel's slices, used the same way (the gradient slice holds each seed's
// stage sources, the per-obstacle curvature serves the obstacle centres' entries of pbar).
// Chunks as the products kernel's; every solver class's workspace holds at least one slice
// (static_assert in nmpc_adjoint.hip).
constexpr int kAdjWs = kPprodWs;

// What the three kernels at a solve's point (x*, lam_g*, lam_x*) take alike (nmpc_point.hip):
// DEVICE pointers, layouts and leading dimensions as nmpc_solve_adjoint_batch_dev
// (include/nmpc_amd.h).  x, p, lam_g, lam_x and the four bounds are required; g, info and delta
// may be null
struct PointIO {
  const double *x, *p, *lam_g, *lam_x, *g, *lbx, *ubx, *lbg, *ubg;
  long long ld_x, ld_p, ld_lam_g, ld_lam_x, ld_g, ld_lbx, ld_ubx, ld_lbg, ld_ubg;
  int* info;
  double* delta;
  double* ws;  // B x kPointWs doubles of the handle's workspace
};

// Per-scenario workspace of those kernels: the KKT kernel's slices, used the same way (the
// gradient slice also holds each seed's stage sources or each direction's h_k, as in the
// adjoint- and parameter-products kernels), the row weights sigma_s and one seed's row seed
// y = sigma_s (lam_g_bar - J q) or one direction's jp = (dg/dp) dp.  Once the factorisation
// stands the stage summaries' slice holds the unit-weight stage-cost gradients that serve a cost
// weight taken from p (6 + 6 per stage) and one direction's state tangent (dX/dp) dp (8 per
// stage).  The per-obstacle curvature lam_{k,o} Hg_o of the products kernels is recomputed from
// X and the centres where a centre comes from p, so the union stays within every solver class's
// workspace (static_assert in nmpc_point.hip).
constexpr int kPointSg = kKktWs;
constexpr int kPointY = kPointSg + (5 + NMPC_MAX_OBS) * kEvalStages;
constexpr int kPointWs = kPointY + (5 + NMPC_MAX_OBS) * kEvalStages;
constexpr int kPointUw = kKktQs;
constexpr int kPointXi = kPointUw + 12 * kEvalStages;

// nmpc_solve_adjoint_batch_dev's own arguments: one of the seeds x_bar / lam_g_bar / X_bar and
// one of pbar / q are required
struct SadjIO {
  PointIO pt;
  const double *x_bar, *lam_g_bar, *X_bar;
  long long ld_x_bar, ld_lam_g_bar, ld_X_bar;
  int na;
  double *pbar, *q, *jq;
};

// nmpc_solve_tangent_batch_dev's own arguments: dp is required, and one of dx / dlam_g / dX
struct StanIO {
  PointIO pt;
  const double* dp;
  long long ld_dp;
  int nd;
  double *dx, *dlam_g, *dX;
};

// nmpc_solve_policy_batch_dev's own arguments: dp where nd > 0, and one of K / kff / A / Bm
struct SpolIO {
  PointIO pt;
  const double* dp;
  long long ld_dp;
  int nd;
  double *K, *kff, *A, *Bm, *X;
};

// DEVICE pointers, layouts and leading dimensions as nmpc_policy_rollout_batch_dev
// (include/nmpc_amd.h); p, ubar, Xbar and e0 are required, lbg and ubg come together, and one of
// J / viol / X / U.  No workspace: each sample's state lives in LDS
struct RollIO {
  const double *p, *ubar, *Xbar, *K, *lbx, *ubx, *lbg, *ubg, *e0, *w;
  long long ld_p, ld_ubar, ld_Xbar, ld_K, ld_lbx, ld_ubx, ld_lbg, ld_ubg, ld_e0, ld_w;
  double *J, *viol;
  int* nsat;
  double *X, *U;
};

// DEVICE pointers, layouts and leading dimensions as nmpc_policy_rollout_adjoint_batch_dev
// (include/nmpc_amd.h); p, ubar, Xbar and X are required, one of the seeds Jb / Xb / Ub and one of
// the six double outputs; K_bar and Xbar_bar only with K
struct RollAdjIO {
  const double *p, *ubar, *Xbar, *K, *lbx, *ubx, *X, *Jb, *Xb, *Ub;
  long long ld_p, ld_ubar, ld_Xbar, ld_K, ld_lbx, ld_ubx, ld_X, ld_Jb, ld_Xb, ld_Ub;
  double *ubar_bar, *K_bar, *Xbar_bar, *p_bar, *e0_bar, *w_bar;
  int* nsat;
  double* ws;  // M > 64 only: B x ceil(M / 64) x (nw + nu nx N + nx (N+1) + np) doubles of the handle's workspace
};

// DEVICE pointers, layouts and leading dimensions as nmpc_policy_covariance_batch_dev
// (include/nmpc_amd.h); p, ubar, Xbar and S0 are required, and one of Sigma / sigma_u / sigma_g.
// No workspace: each case's matrices live in LDS
struct CovIO {
  const double *p, *ubar, *Xbar, *K, *S0, *W, *obs_var;
  long long ld_p, ld_ubar, ld_Xbar, ld_K, ld_S0, ld_W, ld_obs_var;
  double *Sigma, *sigma_u, *sigma_g;
};

// DEVICE pointers, layouts and leading dimensions as nmpc_policy_covariance_adjoint_batch_dev
// (include/nmpc_amd.h); p, ubar, Xbar and Sigma are required, one of the seeds Sigma_bar / var_u_bar /
// var_g_bar and one of the eight outputs; K_bar only with K.  No workspace
struct CovAdjIO {
  const double *p, *ubar, *Xbar, *K, *Sigma, *Sigma_bar, *var_u_bar, *var_g_bar;
  long long ld_p, ld_ubar, ld_Xbar, ld_K, ld_Sigma, ld_Sigma_bar, ld_var_u_bar, ld_var_g_bar;
  double *S0_bar, *W_bar, *Lambda, *obs_var_bar, *K_bar, *ubar_bar, *Xbar_bar, *p_bar;
};

// DEVICE pointers, layouts and leading dimensions as nmpc_policy_value_batch_dev
// (include/nmpc_amd.h); p, ubar and Xbar are required, S0 with nc > 0, and one of J / lam / P / dJ /
// varJ (dJ and varJ only with nc > 0).  Workspace: one products-kernel slice per scenario
// (Solver::derivs writes the stage costs' gradients and Hessians through global pointers)
struct ValIO {
  const double *p, *ubar, *Xbar, *K, *S0, *W;
  long long ld_p, ld_ubar, ld_Xbar, ld_K, ld_S0, ld_W;
  double *J, *lam, *P, *dJ, *varJ;
  double* ws;  // B x kProdWs doubles of the handle's workspace
};

}  // namespace nmpc_impl

// Enqueues the cost-to-go expansions of B scenarios on `stream`: B wavefronts, one per scenario, the
// nc cases a loop at its end.  Same contract as nmpc_eval_launch.
int nmpc_policy_value_launch(const nmpc_impl::Params* dprm, int B, int nc, const nmpc_impl::ValIO& io,
                             void* stream);

// Enqueues the reverse sweep of the closed-loop covariances of B scenarios x nc cases on `stream`:
// B x nc wavefronts laid out as nmpc_policy_covariance_launch's.  Same contract as nmpc_eval_launch.
int nmpc_policy_covariance_adjoint_launch(const nmpc_impl::Params* dprm, int B, int nc,
                                          const nmpc_impl::CovAdjIO& io, void* stream);

// Enqueues the closed-loop covariances of B scenarios x nc cases on `stream`: B x nc wavefronts,
// one per (scenario, case), lane = entry of the 8 x 8 matrix.  Same contract as nmpc_eval_launch.
int nmpc_policy_covariance_launch(const nmpc_impl::Params* dprm, int B, int nc, const nmpc_impl::CovIO& io,
                                  void* stream);

// Enqueues the reverse sweep of the policy rollouts of B scenarios x M samples on `stream`:
// B x ceil(M / 64) wavefronts laid out as nmpc_policy_rollout_launch's and, with more than one
// block of samples, a second kernel that adds the blocks' partial sums (nred doubles per block) in
// block order.  Same contract as nmpc_eval_launch.
int nmpc_policy_rollout_adjoint_launch(const nmpc_impl::Params* dprm, int B, int M, const nmpc_impl::RollAdjIO& io,
                                       int nred, void* stream);

// Enqueues the policy rollouts of B scenarios x M samples on `stream`: B x ceil(M / 64)
// wavefronts, sample s of scenario b on lane s % 64 of wavefront (b, s / 64).  Same contract as
// nmpc_eval_launch.
int nmpc_policy_rollout_launch(const nmpc_impl::Params* dprm, int B, int M, const nmpc_impl::RollIO& io,
                               void* stream);

// Enqueues the feedback policies of B scenarios on `stream` (one wavefront per scenario, every
// direction on it: the factorisation is done once).  Same contract as nmpc_eval_launch.
int nmpc_solve_policy_launch(const nmpc_impl::Params* dprm, int B, const nmpc_impl::SpolIO& io, void* stream);

// Enqueues the fused forward-mode solution sensitivities of B scenarios on `stream` (one
// wavefront per scenario, every direction on it: the factorisation is done once).  Same
// contract as nmpc_eval_launch.
int nmpc_solve_tangent_launch(const nmpc_impl::Params* dprm, int B, const nmpc_impl::StanIO& io, void* stream);

// Enqueues the fused reverse-mode solution sensitivities of B scenarios on `stream` (one
// wavefront per scenario, every seed on it: the factorisation is done once).  Same contract as
// nmpc_eval_launch.
int nmpc_solve_adjoint_launch(const nmpc_impl::Params* dprm, int B, const nmpc_impl::SadjIO& io, void* stream);

// Enqueues the adjoint products of B scenarios on `stream`: B x chunks wavefronts, wavefront
// (b, c) forming scenario b's seeds c, c + chunks, ...  Same contract as nmpc_eval_launch.
int nmpc_adjoint_launch(const nmpc_impl::Params* dprm, int B, int chunks, const nmpc_impl::AdjIO& io,
                        void* stream);

// Enqueues the parameter-direction products of B scenarios on `stream`: B x chunks wavefronts,
// wavefront (b, c) forming scenario b's directions c, c + chunks, ... and wavefront (b, 0) the
// gradient grad_p L.  Same contract as nmpc_eval_launch.
int nmpc_pproducts_launch(const nmpc_impl::Params* dprm, int B, int chunks, const nmpc_impl::PprodIO& io,
                          void* stream);

// Enqueues the KKT solves of B scenarios on `stream` (one wavefront per scenario, every
// right-hand side on it: another wavefront would repeat the factorisation).  Same contract as
// nmpc_eval_launch.
int nmpc_kkt_launch(const nmpc_impl::Params* dprm, int B, const nmpc_impl::KktIO& io, void* stream);

// Enqueues the evaluation of B scenarios on `stream` (one wavefront per scenario); returns
// the hipError_t of the launch.  No allocation, no synchronisation.
int nmpc_eval_launch(const nmpc_impl::Params* dprm, int B, const nmpc_impl::EvalIO& io, void* stream);

// Enqueues the Jacobian- / Hessian-vector products of B scenarios on `stream`: B x chunks
// wavefronts, wavefront (b, c) forming scenario b's directions c, c + chunks, ...  Same
// contract as nmpc_eval_launch.
int nmpc_products_launch(const nmpc_impl::Params* dprm, int B, int chunks, const nmpc_impl::ProdIO& io,
                         void* stream);

#endif  // NMPC_EVAL_H
