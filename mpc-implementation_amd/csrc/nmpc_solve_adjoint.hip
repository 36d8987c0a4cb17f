// nmpc_solve_adjoint.hip -- the reverse-mode sensitivity of a SOLUTION in one launch
// (nmpc_solve_adjoint_batch / nmpc_solve_adjoint_batch_dev, include/nmpc_amd.h): for each of B
// scenarios at a solve's (x*, lam_g*, lam_x*) and each of na seeds (x_bar on x*, lam_g_bar on
// lam_g*, X_bar on X*), with the barrier weights Sigma_x, Sigma_s of the point and
//   M = W + diag(Sigma_x) + delta I + J^T diag(Sigma_s + delta) J,
//   q = M^-1 (x_bar + (dX/dw)^T X_bar + J^T Sigma_s lam_g_bar),
//   pbar = -(d_p grad_w L)^T q + (dg/dp)^T Sigma_s (lam_g_bar - J q) + (dX/dp)^T X_bar
// so that <pbar, dp> = <x_bar, dx*> + <lam_g_bar, dlam_g*> + <X_bar, dX*> for every dp.  What
// Solver.sensitivity_adjoint composes on the host from three launches of nmpc_adjoint.hip and
// nmpc_kkt.hip, the weights in NumPy and the delta ladder as a Python loop, on the device.
//
// Part of the evaluation kernel's translation unit (nmpc_eval.hip includes this file after
// nmpc_point.hip), so everything is the text the solver compiles; the LDS carve-up, the
// workspace slices and the steps up to the factorisation are nmpc_point.hip's, shared with
// nmpc_solve_tangent.hip and nmpc_solve_policy.hip.
//
// Execution model: the siblings'.  One wavefront per scenario, fp64, stage k on lane k, rows
// and variables strided over the lanes, control flow wave-uniform.
// Once per wavefront:
//   1. load_params, load_controls, point_rollout: scenario data, rollout and stage costs;
//   2. point_weights: the barrier weights; an equality row, lbx > ubx or a weight that is not a
//      finite non-negative number ends the scenario with info = -11 and NaN outputs;
//      point_derivs: gl, Hl, lam_{k+1};
//   3. lane k keeps the second-order data every seed's pullback needs: the summed obstacle
//      curvature and the dynamics terms d33, d34, d44, s03, s04 of lam_{k+1}^T T f (stage 0's
//      included: its Hxu_0 z_0 reaches the x0 block of pbar);
//   4. point_ladder: the stage summaries and Solver::riccati up the delta ladder; beyond
//      max_hessian_perturbation info = 1 and NaN outputs.  point_unit_grads where a cost weight
//      comes from p.
// Per seed (the factorisation is shared):
//   5. r_w = x_bar + (dX/dw)^T X_bar -- with X_bar, one reverse sweep (Solver::adjoint on the
//      stage sources X_bar_k, grad_u) -- and q_k = -G_k^T (sigma_s lam_g_bar);
//   6. Solver::resolve, Solver::forward: q, and its state step dX = (dX/dw) q; J q by row_jd;
//   7. y = sigma_s (lam_g_bar - J q) into the workspace, z = -q;
//   8. the pullback of (y, z, X_bar) to p as nmpc_adjoint_kernel's steps 6 to 9, with the
//      tangent of z taken from the forward sweep (xi = -dX: no second prefix-sum tangent) and an
//      obstacle's own curvature lam_{k,o} Hg_o recomputed where its centre comes from p.
// Every per-seed buffer is rewritten by each seed, so the seeds are independent.
// (included by nmpc_eval.hip)

namespace {

__global__ __launch_bounds__(WAVE) void nmpc_solve_adjoint_kernel(const Params* __restrict__ prm, int B, SadjIO io) {
  __shared__ __attribute__((aligned(16))) double smem[A_TOTAL];
  const int b = blockIdx.x;
  if (b >= B) return;
  Solver<CapEv> S{};
  LDS double* sm = (LDS double*)smem;
  const PointRefs R = point_bind(S, prm, sm, io.pt, b);
  GLB double *rv = R.rv, *dU = R.dU, *sg = R.sg, *yv = R.yv, *uw = R.uw;
  LDS double* dX = sm + B_INC;
  const int N = S.N, m = S.m, nb = S.nb, nw = S.nw, ng = S.ng, nwE = S.nwE;
  const int np = prm->np, npE = prm->npE, nxE = prm->nxE, nXE = nxE * (N + 1);
  const int w1p = prm->w1p, w2p = prm->w2p;
  const double T = S.T;
  const int lane = S.lanef();
  const double* yb = R.yb;
  const double* xs = io.x_bar ? io.x_bar + (long long)b * io.ld_x_bar : nullptr;
  const double* ls = io.lam_g_bar ? io.lam_g_bar + (long long)b * io.ld_lam_g_bar : nullptr;
  const double* Xs = io.X_bar ? io.X_bar + (long long)b * io.ld_X_bar : nullptr;

  // every output of the scenario NaN (wave-uniform callers), its verdict and delta out
  auto finish_nan = [&](int verdict, double delta) {
    const long long na = io.na;
    nan_fill(io.pbar ? io.pbar + (long long)b * na * npE : nullptr, na * npE, lane);
    nan_fill(io.q ? io.q + (long long)b * na * nwE : nullptr, na * nwE, lane);
    nan_fill(io.jq ? io.jq + (long long)b * na * ng : nullptr, na * ng, lane);
    point_verdict(S, io.pt, lane, verdict, delta);
  };

  load_params(S, prm, lane, io.pt.p + (long long)b * io.pt.ld_p);
  load_controls(S, prm, lane, R.xb, true);
  sync();
  point_rollout(S, lane);

  const int k = lane;
  const bool stage = k >= 1 && k <= N;  // the stages whose state depends on w
  const int sv[6] = {0, 1, 2, 5, 6, 7};  // the states a stage cost reads

  if (point_weights(S, prm, R, k)) {
    finish_nan(-11, 0.0);
    return;
  }
  point_derivs(S, R);

  // ---------------- lane k: the second-order data of every seed's pullback, in registers.  Not
  // point_curvature: the curvature of stages k >= 1 alone, only where pbar is wanted, its sum
  // open to contraction, and the dynamics terms added to zeros as a stage summary adds them
  double q00 = 0.0, q01 = 0.0, q11 = 0.0;
  double d33 = 0.0, d34 = 0.0, d44 = 0.0, s03 = 0.0, s04 = 0.0;  // (stage 0's s03, s04 are not in qs)
  if (io.pbar) {
    if (stage) {  // lam_g-weighted obstacle curvature: nmpc_adjoint_kernel's, rows in order
      for (int o = 0; o < S.nobs; ++o) {
        const ObsCurv h = obstacle_curvature(S, k, o, yb[k * m + nb + o]);
        q00 += h.h00; q01 += h.h01; q11 += h.h11;
      }
    }
    if (k < N) {
      const Dyn2 e = point_dyn2(S, k);
      d33 += T * e.e33; d44 += T * e.e44; d34 += T * e.e34;
      s03 = T * e.e03; s04 = T * e.e04;
    }
  }

  double delta;
  if (const int verdict = point_ladder(S, prm, R, k, 0.0, 0.0, delta)) {
    finish_nan(verdict, delta);
    return;
  }
  sync();
  point_verdict(S, io.pt, lane, 0, delta);
  if (io.pbar) point_unit_grads(S, prm, R, lane);

  // the internal entry of p this lane forms, and its place in the caller's layout
  const int pe = lane < np ? ext_p(prm, lane) : -1;

  // ---------------- seeds
  for (int d = 0; d < io.na; ++d) {
    const double* xd = xs ? xs + (long long)d * nwE : nullptr;
    const double* ld = ls ? ls + (long long)d * ng : nullptr;
    const double* Xd = Xs ? Xs + (long long)d * nXE : nullptr;
    // 5. r_k = -(x_bar + (dX/dw)^T X_bar), q_k = -G_k^T (sigma_s lam_g_bar)
    if (Xd) {
      if (k <= N) {
        GLB double* h = S.gl + k * 8;
#pragma unroll
        for (int c = 0; c < 8; ++c) h[c] = c < nxE ? Xd[k * nxE + c] : 0.0;
      }
      sync();
      S.adjoint(1.0, (const double*)nullptr);
    }
    for (int i = lane; i < nw; i += WAVE) {
      const int e = ext_u(prm, i);
      double r = 0.0;
      if (e >= 0) {
        if (Xd) {
          const double g = S.grad_u(i);
          r = -(xd ? xd[e] + g : g);
        } else if (xd) {
          r = -xd[e];
        }
      }
      rv[i] = r;
    }
    if (stage) {
      const LDS double* xk = S.X + k * 8;
      double q8[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) q8[c] = 0.0;
      if (ld) {
        double qx = 0.0, qy = 0.0;
        for (int i = 0; i < m; ++i) {
          const double rg = sg[k * m + i] * ld[k * m + i];
          const double t = -rg;
          if (i < nb) {
            const int bi = boxidx(i);
#pragma unroll
            for (int c = 2; c < 8; ++c) q8[c] = c == bi ? t : q8[c];
          } else {
            const int o = i - nb;
            const double ddx = xk[0] - S.obx[o], ddy = xk[1] - S.oby[o];
            const double idd = rsq(ddx * ddx + ddy * ddy);
            qx += t * (-(ddx * idd));
            qy += t * (-(ddy * idd));
          }
        }
        q8[0] = qx;
        q8[1] = qy;
      }
      LDS double* qo = S.qs + k * 10;
#pragma unroll
      for (int c = 0; c < 8; ++c) qo[c] = q8[c];
    }
    sync();
    // 6. the solves: q and its state step
    S.resolve(rv);
    S.forward(dU, dX);
    if (io.q) {
      double* o = io.q + ((long long)b * io.na + d) * nwE;
      for (int i = lane; i < nw; i += WAVE) {
        const int e = ext_u(prm, i);
        if (e < 0) continue;
        o[e] = S.fixed(i) ? 0.0 : dU[i];
      }
    }
    // 7. J q, and y = sigma_s (lam_g_bar - J q) (stage 0's rows: J is zero there)
    {
      double* o = io.jq ? io.jq + ((long long)b * io.na + d) * ng : nullptr;
      for (int r = lane; r < ng; r += WAVE) {
        const double jq = r < m ? 0.0 : S.row_jd(r, dX);
        if (o) o[r] = jq;
        // (the difference first: on an active row sigma_s is large and J q close to lam_g_bar)
        yv[r] = ld ? sg[r] * (ld[r] - jq) : -(sg[r] * jq);
      }
    }
    if (!io.pbar) {
      sync();
      continue;
    }
    // 8. the pullback (nmpc_adjoint_kernel's steps 6 to 9 with z = -q, xi = -(dX/dw) q)
    double dx[8], du0 = 0.0;
#pragma unroll
    for (int c = 0; c < 8; ++c) dx[c] = k <= N ? -dX[k * 8 + c] : 0.0;
    if (k < N) du0 = S.fixed(k * 6) ? -0.0 : -dU[k * 6];
    double t0 = 0.0, t1 = 0.0;  // (Hl_k xi_k)[0:2]: the target's part of pbar
    if (k <= N) {
      double hs[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) hs[c] = 0.0;
      if (stage) {
#pragma unroll
        for (int a = 0; a < 6; ++a) {
          double acc = 0.0;
#pragma unroll
          for (int q = 0; q < 6; ++q) acc += S.Hl[k * 21 + hp(a, q)] * dx[sv[q]];
          hs[sv[a]] = acc;
        }
        if (k < N) { t0 = hs[0]; t1 = hs[1]; }
        if (S.nobs > 0) {
          hs[0] += q00 * dx[0] + q01 * dx[1];
          hs[1] += q01 * dx[0] + q11 * dx[1];
        }
        // (stage N: no dynamics follow it, its terms are absent)
        hs[3] = k < N ? (d33 * dx[3] + d34 * dx[4]) + s03 * du0 : 0.0;
        hs[4] = k < N ? (d34 * dx[3] + d44 * dx[4]) + s04 * du0 : 0.0;
      } else {  // stage 0: Hxu_0 z_0 alone
        hs[3] = k < N ? s03 * du0 : 0.0;
        hs[4] = k < N ? s04 * du0 : 0.0;
      }
      if (Xd) {
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          if (c < nxE) hs[c] = hs[c] + Xd[k * nxE + c];
        }
      }
      GLB double* h = S.gl + k * 8;
#pragma unroll
      for (int c = 0; c < 8; ++c) h[c] = hs[c];
    }
    sync();
    // nu_k = s_k + G_k^T y_k + A_k^T nu_{k+1}
    S.adjoint(1.0, (const GLB double*)yv);
    // pbar, lane i forming internal entry i
    {
      double v = lane < 8 ? S.lam[lane] : 0.0;
      const double gxt = -wsum(t0);
      const double gyt = -wsum(t1);
      if (lane == 8) v = gxt;
      else if (lane == 9) v = gyt;
      if (w1p >= 0) {
        double a_ = 0.0;
        if (stage && k < N) {
#pragma unroll
          for (int a = 0; a < 6; ++a) a_ += uw[k * 12 + a] * dx[sv[a]];
        }
        const double s = wsum(a_);
        if (lane == w1p) v += s;
      }
      if (w2p >= 0) {
        double a_ = 0.0;
        if (stage && k < N) {
#pragma unroll
          for (int a = 0; a < 6; ++a) a_ += uw[k * 12 + 6 + a] * dx[sv[a]];
        }
        const double s = wsum(a_);
        if (lane == w2p) v += s;
      }
      for (int o = 0; o < S.nobs; ++o) {
        const int ix = prm->oxp[o], iy = prm->oyp[o];
        if (ix < 0 && iy < 0) continue;
        double cx = 0.0, cy = 0.0;
        if (k <= N) {  // row g = r_sum - |(x, y) - (ox, oy)|: dg/dox = (x - ox) / d
          const double yo = yv[k * m + nb + o];
          const LDS double* xk = S.X + k * 8;
          const double ddx = xk[0] - S.obx[o], ddy = xk[1] - S.oby[o];
          const double idd = rsq(ddx * ddx + ddy * ddy);
          cx = yo * (ddx * idd);
          cy = yo * (ddy * idd);
          if (stage) {  // the centre's move against the obstacle's own curvature, recomputed
            const double C = yb[k * m + nb + o];
            const double id3 = idd * idd * idd;
            const double h00 = C * (-ddy * ddy * id3), h01 = C * (ddx * ddy * id3), h11 = C * (-ddx * ddx * id3);
            cx -= h00 * dx[0] + h01 * dx[1];
            cy -= h01 * dx[0] + h11 * dx[1];
          }
        }
        cx = wsum(cx); cy = wsum(cy);
        if (lane == ix) v += cx;
        if (lane == iy) v += cy;
      }
      if (pe >= 0) io.pbar[((long long)b * io.na + d) * npE + pe] = v;
    }
    sync();
  }
}

}  // namespace

int nmpc_solve_adjoint_launch(const Params* dprm, int B, const SadjIO& io, void* stream) {
  hipLaunchKernelGGL(nmpc_solve_adjoint_kernel, dim3(B), dim3(WAVE), 0, (hipStream_t)stream, dprm, B, io);
  return (int)hipGetLastError();
}
