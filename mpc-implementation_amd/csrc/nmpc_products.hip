// nmpc_products.hip -- batched Jacobian- and Hessian-vector products at GIVEN points
// (nmpc_products_batch / nmpc_products_batch_dev, include/nmpc_amd.h): for each of B
// scenarios and each of nv directions v in decision space
//   J_g(x, p) v,   (obj_factor grad^2 f + sum_i lam_g_i grad^2 g_i) v,   (dX/dw) v
// CasADi's nlp_jac_g and nlp_hess_l applied to a vector; oracle SSEval.J, SSEval.hessian
// and SSEval.Z without forming Z.
//
// Part of the evaluation kernel's translation unit: nmpc_eval.hip includes this file after
// its own kernel, so the solver's source is seen with no class selected and the second
// derivatives here are the text the solver compiles -- Solver::derivs<true> (Hl),
// Solver::adjoint (the dynamics multipliers, and again for the sweep over h), the obstacle
// curvature and the five dynamics terms of Solver::assemble, Solver::row_jd, Solver::grad_u.
//
// Execution model: the solver's.  One wavefront per (scenario, direction chunk), stage k on
// lane k, rows and decision variables strided over the lanes, control flow wave-uniform.
// Once per wavefront:
//   1. scenario data, rollout and stage costs (load_params, load_controls, point_rollout of
//      nmpc_eval_shared.hip: the stage costs fill the transcendental cache that
//      derivs<true, true> reads);
//   2. derivs<true, true>: gl, Hl; adjoint(obj_factor, lam_g): lam_{k+1};
//   3. lane k keeps its stage's second-order data in registers for every direction:
//      Hq = obj_factor Hl_k + sum_o lam_{k,o} Hg_o (21 packed entries over x, y, z, x5, x6, x7),
//      the dynamics terms d33, d34, d44 (theta, psi) and s03, s04 (theta / psi against v) of
//      lam_{k+1}^T T f (k < N), and the entries of A_k = I + E_k and of B_k's first column.
// Per direction (forward over reverse):
//   4. tangent rollout dX_0 = 0, dX_{k+1} = A_k dX_k + B_k du_k as in-order prefix sums, the
//      angles first and then the positions, as Solver::rollout;
//   5. J v: row (k, i) = G_{k,i} dX_k (Solver::row_jd), rows strided over the lanes;
//   6. h_k = Hxx_k dX_k + Hxu_k du_k (k >= 1) into the gradient slice of the workspace;
//   7. mu_k = h_k + A_k^T mu_{k+1}: Solver::adjoint(1, no rows) on that slice;
//   8. (W v)_{u_k} = B_k^T mu_{k+1} (Solver::grad_u) + Hxu_k^T dX_k.
// Stage 0 is constant in w: dX_0 and its rows are written as 0 and its terms are never
// formed (no 0 * NaN).  Every per-direction buffer is rewritten by each direction, and a
// lane's sums take only the stages its result depends on, so directions are independent and
// the results do not depend on how the directions are dealt to wavefronts.
// (included by nmpc_eval.hip)

namespace {

static_assert(fits_every_class(kProdWs),
              "a solver class's workspace is smaller than one wavefront's of the products kernel");

// LDS carve-up (doubles): the unit's head (its multipliers' buffer holds lam, then each
// direction's mu), then
constexpr int P_DX = B_END;                   // the direction's tangent trajectory
constexpr int P_CR = P_DX + 8 * NS;           // the direction's Hxu_k^T dX_k
constexpr int P_TOTAL = P_CR + NS;
static_assert(P_TOTAL * 8 <= 32 * 1024, "products kernel LDS");

__global__ __launch_bounds__(WAVE) void nmpc_products_kernel(const Params* __restrict__ prm, int B, int chunks,
                                                             ProdIO io) {
  __shared__ __attribute__((aligned(16))) double smem[P_TOTAL];
  const int b = blockIdx.x, chunk = blockIdx.y;
  if (b >= B) return;
  Solver<CapEv> S{};
  LDS double* sm = (LDS double*)smem;
  GLB double* gw = (GLB double*)(io.ws + ((long long)b * chunks + chunk) * kProdWs);
  bind_solver(S, prm, sm, gw, b, kProdU, kProdGl, kProdHl, kProdTc, kProdDc);
  LDS double* dX = sm + P_DX;
  LDS double* cr = sm + P_CR;
  const int N = S.N, m = S.m, nb = S.nb, ng = S.ng, nwE = S.nwE;
  const int nXE = prm->nxE * (N + 1);
  const double T = S.T;
  const int lane = S.lanef();
  const double* yb = io.lam_g ? io.lam_g + (long long)b * io.ld_lam_g : nullptr;
  const double* vb = io.v + (long long)b * io.ld_v;

  // ---------------- scenario data, rollout, stage costs, derivatives, multipliers
  load_params(S, prm, lane, io.p + (long long)b * io.ld_p);
  load_controls(S, prm, lane, io.x + (long long)b * io.ld_x, true);
  sync();
  point_rollout(S, lane);
  S.derivs<true, true>(S.X, S.U, S.tc);
  if (yb) S.adjoint(io.obj_factor, yb);
  else S.adjoint(io.obj_factor, (const double*)nullptr);

  // ---------------- lane k: stage k's second-order data, kept in registers
  const int k = lane;
  const bool stage = k >= 1 && k <= N;  // the stages whose state depends on w
  double Hq[21];
#pragma unroll
  for (int t = 0; t < 21; ++t) Hq[t] = 0.0;
  double d33 = 0.0, d34 = 0.0, d44 = 0.0, s03 = 0.0, s04 = 0.0;
  const StageAB ab = point_stage_ab(S, k);
  if (stage) {
#pragma unroll
    for (int t = 0; t < 21; ++t) Hq[t] = io.obj_factor * S.Hl[k * 21 + t];
    if (yb) {  // y-weighted obstacle curvature, rows in order; the sum is open to contraction
      double q00 = 0.0, q01 = 0.0, q11 = 0.0;
      for (int o = 0; o < S.nobs; ++o) {
        const ObsCurv h = obstacle_curvature(S, k, o, yb[k * m + nb + o]);
        q00 += h.h00; q01 += h.h01; q11 += h.h11;
      }
      if (S.nobs > 0) { Hq[hp(0, 0)] += q00; Hq[hp(0, 1)] += q01; Hq[hp(1, 1)] += q11; }
    }
    if (k < N) {
      const Dyn2 e = point_dyn2(S, k);
      d33 = T * e.e33; d44 = T * e.e44; d34 = T * e.e34;
      s03 = T * e.e03; s04 = T * e.e04;
    }
  }
  sync();  // lam is rewritten by every direction's sweep

  // ---------------- directions c, c + chunks, ...
  for (int d = chunk; d < io.nv; d += chunks) {
    // 4. tangent rollout
    const double* vd = vb + (long long)d * nwE;
    double du[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) du[c] = (k < N && c < S.nuE) ? vd[k * S.nuE + c] : 0.0;
    if (k < N) {
#pragma unroll
      for (int c = 0; c < 5; ++c) S.inc[k * 8 + c] = T * du[1 + c];
    }
    sync();
    double dx[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) dx[c] = 0.0;
    if (k <= N) {
      for (int j = 0; j < k; ++j) {
#pragma unroll
        for (int c = 0; c < 5; ++c) dx[3 + c] = dx[3 + c] + S.inc[j * 8 + c];
      }
      if (k < N) {  // stage 0: dX_0 = 0, only B_0 du_0
        S.inc[k * 8 + 5] = k == 0 ? ab.b00 * du[0] : (ab.E03 * dx[3] + ab.E04 * dx[4]) + ab.b00 * du[0];
        S.inc[k * 8 + 6] = k == 0 ? ab.b10 * du[0] : (ab.E13 * dx[3] + ab.E14 * dx[4]) + ab.b10 * du[0];
        S.inc[k * 8 + 7] = k == 0 ? ab.b20 * du[0] : ab.E23 * dx[3] + ab.b20 * du[0];
      }
    }
    sync();
    if (k <= N) {
      for (int j = 0; j < k; ++j) {
        dx[0] = dx[0] + S.inc[j * 8 + 5];
        dx[1] = dx[1] + S.inc[j * 8 + 6];
        dx[2] = dx[2] + S.inc[j * 8 + 7];
      }
#pragma unroll
      for (int c = 0; c < 8; ++c) dX[k * 8 + c] = dx[c];
    }
    // 6. h_k, and the cross term of step 8
    if (k <= N) {
      GLB double* h = S.gl + k * 8;
      if (stage) {
        const int sv[6] = {0, 1, 2, 5, 6, 7};
#pragma unroll
        for (int a = 0; a < 6; ++a) {
          double acc = 0.0;
#pragma unroll
          for (int q = 0; q < 6; ++q) acc += Hq[hp(a, q)] * dx[sv[q]];
          h[sv[a]] = acc;
        }
        // (stage N: no dynamics follow it, its terms are absent)
        h[3] = k < N ? (d33 * dx[3] + d34 * dx[4]) + s03 * du[0] : 0.0;
        h[4] = k < N ? (d34 * dx[3] + d44 * dx[4]) + s04 * du[0] : 0.0;
        cr[k] = k < N ? s03 * dx[3] + s04 * dx[4] : 0.0;
      } else {
#pragma unroll
        for (int c = 0; c < 8; ++c) h[c] = 0.0;
        cr[k] = 0.0;
      }
    }
    sync();
    // 5. J v and the tangent out
    if (io.jv) put_rows_jd(S, lane, dX, io.jv + ((long long)b * io.nv + d) * ng);
    if (io.dX) put_trajectory(prm, lane, dX, io.dX + ((long long)b * io.nv + d) * nXE);
    if (!io.hv) {
      sync();
      continue;
    }
    // 7. mu_k = h_k + A_k^T mu_{k+1}
    S.adjoint(1.0, (const double*)nullptr);
    // 8. (W v)_{u_k}: stage 0's cross term is absent
    put_grad_u(S, prm, lane, cr, true, false, io.hv + ((long long)b * io.nv + d) * nwE);
    sync();
  }
}

}  // namespace

int nmpc_products_launch(const Params* dprm, int B, int chunks, const ProdIO& io, void* stream) {
  hipLaunchKernelGGL(nmpc_products_kernel, dim3(B, chunks), dim3(WAVE), 0, (hipStream_t)stream, dprm, B, chunks, io);
  return (int)hipGetLastError();
}
