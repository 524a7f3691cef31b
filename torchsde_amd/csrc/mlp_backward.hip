// Gradient of the perceptron-drift trajectory kernel (mlp_trajectory.hip), Euler-Maruyama: back-propagation through
// the solver, the gradient `loss.backward()` yields when autograd records torchsde's stepping loop
// (base_solver.py:114-134 with euler.py:31-36) -- as two kernels instead of a tape of ~20 torch ops per step.
//
//   step k (forward):   z = W1 y_k + b1,  h = act(z),  f = W2 h + b2,  g = c*y_k + e,
//                       y_{k+1} = y_k + f dt_k + g dW_k
//   step k (reverse):   lam = dL/dy_{k+1}
//                       u     = W2^T lam                 delta = u * act'(z) * dt_k
//                       dL/dy_k = lam + W1^T delta + lam * c * dW_k
//                       dL/dW2 += (dt_k lam) h^T         dL/dW1 += delta y_k^T
//                       dL/db2 += dt_k lam               dL/db1 += delta
//                       dL/dc  += lam * y_k * dW_k       dL/de  += lam * dW_k
//   Milstein (milstein.py:52-74 for this g: gdg = g c) adds (g v) c with v = (dW^2 - dt)/2 (Ito) or dW^2/2:
//                       dL/dy_k += lam c^2 v             dL/dc += lam v (g + c y_k)       dL/de += lam c v
//
// 1. mlp_backward_kernel -- the reverse sweep. A wave owns 16 batch rows for all steps; lam stays in registers in the
//    MFMA accumulator layout (the layout of the sampling kernel: it is the B operand of the next product as it
//    stands); the three products per step run on v_mfma_f32_16x16x4_f32 against the SAME two LDS weight arrays the
//    sampling kernel uses -- layer 1 reads W1 as stored, the two transposed products read 16-byte rows (four
//    consecutive K per lane, one ds_read_b128 feeding four MFMAs; conflict-free with the +4 row padding). The states
//    y_k come from the forward launch (which wrote every step: 288 GB of HBM is what pays for this), dW_k is
//    regenerated from the counter RNG, and the per-step factors of the weight gradients (dt lam, h, delta) are
//    stashed in HBM for:
// 2. gram_kernel -- C = A^T B and the column sums of A over a very tall K (K = steps x batch rows, M, N <= 128): the
//    weight- and bias-gradient sums. Each block owns a contiguous K range and accumulates the whole M x N result in
//    MFMA accumulators across its 8 waves, streaming both operands through a double-buffered LDS tile; per-block
//    partials are written out and summed in a fixed order by the caller (deterministic, unlike atomics).
#include <type_traits>

#include "tsde_common.h"
#include "tsde_launch.h"
#include "tsde_mlp.h"
#include "tsde_schemes.h"

namespace tsde {

struct MlpBackArgs {
  float* lam;               // (B, d)  in: dL/dy at boundary k_hi (before that boundary's own cotangent); out: at k_lo
  float* stash_lam;         // (k_hi - k_lo, B, d)   dt_k * dL/dy_{k+1}
  float* stash_hid;         // (k_hi - k_lo, B, h)   act(W1 y_k + b1)
  float* stash_delta;       // (k_hi - k_lo, B, h)   delta_k
  float* row_rate;          // (B, d)  += sum_k lam * y_k * dW_k   (per trajectory; the caller sums over the batch)
  float* row_shift;         // (B, d)  += sum_k lam * dW_k
  const float* ys_all;      // (.., B, d) states at step boundaries ys_first, ys_first + 1, ... (at least up to k_hi - 1)
  int32_t ys_first;
  const float* grad_ys;     // (n_grad, B, d) cotangents of the outputs
  const int32_t* grad_step; // (n_grad) ascending: output j sits in step grad_step[j] - 1, on boundary grad_step[j] or inside
  const float* grad_w;      // (n_grad, 2) interpolation weights (w0, w1) of each output, or null: every output on its boundary
  int32_t grad_last;        // index of the last output with grad_step <= k_hi (-1: none)
  const float* W1;          // (d, h) as in MlpArgs
  const float* b1;          // (h)
  const float* W2;          // (h, d)
  const float *c, *e;       // (d) diffusion g = c*y + e (e is only read by the Milstein terms)
  int32_t method;           // TSDE_TRAJ_EULER / _MILSTEIN_ITO / _MILSTEIN_STRAT
  int32_t diff_kind;        // TSDE_DIFF_AFFINE / TSDE_DIFF_SIGMOID (the latter with Euler only)
  float diff_amp;
  const float* rows;        // (n_steps, 8)
  const uint32_t* cells;
  int64_t B;
  int32_t d, h;
  int32_t k_lo, k_hi;
  NoiseKey key;
  const uint64_t* key_dev;
};

// The KL instantiation (`sdeint(..., logqp=True)` under autograd, the solve of tsde_trajectory_mlp_diag_logqp with a per-channel
// affine prior drift h = hr * y + hs): the forward step also advanced the column l_{k+1} = l_k + 0.5 sum_i u_i^2 dt_k,
// u = (f - h) / safe(g) at y_k. Its cotangent a_l = dL/dl_{k+1} is per row, gains the column's cotangent where an output
// arrives (as lam gains grad_ys) and is otherwise constant: nothing depends on l. It reaches the rest of the step through
// u -- f = W2 act(z) + b2 is needed again, a fourth product per step from the same LDS copy of W2 -- with (tsde_mlp.h:
// kl_share) w = a_l u / safe per channel:
//   the cotangent fed to the W2 product, and stashed for dL/dW2, dL/db2, is dt (lam + w) instead of dt lam
//   dL/dy_k  += dt (-hr w - a_l u^2 g' / safe)                                  (g' = q c as in the diffusion terms)
//   dL/dc    += -dt a_l (u^2 / safe) q y_k        dL/de += -dt a_l (u^2 / safe) q
//   dL/dhr   += -dt w y_k                          dL/dhs += -dt w
// The replaced divisor (|g| <= 1e-7) is a constant without a derivative. The column's diffusion is 0, so Milstein's own terms
// are unchanged. The Brownian field has row stride d + 1 and any elem0: dW_k comes from normal4_straddle, as the forward kernel
// draws it. The elementwise phase runs BEFORE the W2 product here (it forms that product's operand and then no longer needs f).
struct MlpBackKlArgs : MlpBackArgs {
  float* a_l;               // (B)  in: dL/dl at boundary k_hi (before that boundary's own cotangent); out: at k_lo
  const float* grad_logqp;  // (n_grad, B) cotangents of the column at the outputs
  const float* b2;          // (d)
  const float *hr, *hs;     // (d) prior drift coefficients
  float* row_hrate;         // (B, d)  += sum_k -dt w y_k   (all four sums of this instantiation: over the steps AND over each
  float* row_hshift;        // (B, d)  += sum_k -dt w        aligned group of 16 rows, into row 16 k -- as the adjoint kernel's)
  int64_t bm_stride;        // row stride of the Brownian field: d + 1
};

// FULL: d == D and h == H (no channel padding inside the kernel), which removes every per-tile bounds test.
// KIND (KL only; the plain sweep keeps its uniform branches): which elementwise phase the instantiation holds -- with all of
// them in one kernel behind uniform branches the register allocator spilled hundreds of dwords at every shape.
constexpr int kKlEulerAffine = 0, kKlEulerSigmoid = 1, kKlMilsteinAffine = 2;

// WEIGHTED: outputs anywhere in a step (`grad_w`); without, every output sits on its boundary and `grad_w` is not read -- the
// sweep as it was before outputs inside steps, instruction for instruction.
template <int D, int H, int ACT, int NW, bool FULL, bool KL = false, int KIND = 0, bool WEIGHTED = false>
__global__ void __launch_bounds__(NW * 64)
    mlp_backward_kernel(const std::conditional_t<KL, MlpBackKlArgs, MlpBackArgs> p) {
  constexpr int R = 16;
  using TL = Tile<R>;
  constexpr int TD = D / R, TH = H / R, kThreads = NW * 64;
  using L = MlpLds<R>;
  constexpr int S1 = H + L::kPad, S2 = D + L::kPad;
  extern __shared__ float lds[];
  float* W1s = lds;                         // D rows of S1: W1s[channel][hidden]
  float* W2s = lds + L::w2(D, H);           // H rows of S2: W2s[hidden][channel]
  float* b1s = lds + L::b1(D, H);           // H
  float* cs = lds + L::vec(D, H, 0);        // D
  float* es = lds + L::vec(D, H, 1);        // D
  [[maybe_unused]] float* b2s = lds + L::vec(D, H, 2);      // D  (KL)
  [[maybe_unused]] float* hrs = lds + L::vec(D, H, 3);      // D  (KL) prior drift h = hr * y + hs
  [[maybe_unused]] float* hss = lds + L::vec(D, H, 4);      // D  (KL)
  [[maybe_unused]] float* sums = lds + L::vec(D, H, 5);     // NW x 4 x D  (KL) per wave: rate, shift, prior rate, prior shift
  const int dT = p.d, hT = p.h;
  stage_perceptron<D, H, R, kThreads>(lds, p.W1, p.W2, p.b1, dT, hT);
  for (int i = threadIdx.x; i < D; i += kThreads) {
    cs[i] = i < dT ? p.c[i] : 0.0f;
    es[i] = i < dT ? p.e[i] : 0.0f;
    if constexpr (KL) {
      b2s[i] = i < dT ? p.b2[i] : 0.0f;
      hrs[i] = i < dT ? p.hr[i] : 0.0f;
      hss[i] = i < dT ? p.hs[i] : 0.0f;
    }
  }
  if constexpr (KL) {
    for (int i = threadIdx.x; i < NW * 4 * D; i += kThreads) sums[i] = 0.0f;
  }
  __syncthreads();

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int part = lane / R, n = lane % R;
  // A wave with no batch row left is done; in the last partial wave the surplus lanes shadow the last row: they read
  // what its lane reads, draw the same noise, and (re)write the same values to the same addresses -- no lane masks.
  const int64_t row0 = ((int64_t)blockIdx.x * NW + wave) * R;
  if (row0 >= p.B) return;
  const int64_t row = row0 + n < p.B ? row0 + n : p.B - 1;
  const NoiseKey key = launch_key(p.key, p.key_dev);

  // register r of tile t in this lane = channel 16 t + 4 part + r of batch row `row` (one 16-byte quad per tile).
  // Addresses are a wave-uniform base (SGPRs) + ONE 32-bit lane offset per row width + a constant per tile, so that
  // no per-tile 64-bit address lives in vector registers across the sweep (the caller keeps rows * width < 2^30).
  const uint32_t off_d = (uint32_t)(row * dT) + 4 * part, off_h = (uint32_t)(row * hT) + 4 * part;
  const uint64_t quad0 = (key.elem0 + (uint64_t)(row * dT) + 4 * part) >> 2;   // RNG quad of tile 0; tile t: + 4 t
  // KL: the lane's first element of the field, quad-aligned on every fourth row only (normal4_straddle); a_l of its row
  [[maybe_unused]] uint64_t elem0_lane = 0;
  [[maybe_unused]] float al = 0.0f;
  [[maybe_unused]] const float own_row = row0 + n < p.B ? 1.0f : 0.0f;   // (a shadow lane adds nothing to the wave's sums)
  [[maybe_unused]] float* wave_sums = sums + wave * 4 * D;
  if constexpr (KL) {
    elem0_lane = key.elem0 + (uint64_t)row * (uint64_t)p.bm_stride + 4 * part;
    al = p.a_l[row];
  }
  auto real_d = [&](int t) { return FULL || R * t + 4 * part < dT; };
  auto real_h = [&](int th) { return FULL || R * th + 4 * part < hT; };
  auto load_tile = [&](const float* base, int t) {
    f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (real_d(t)) v = *reinterpret_cast<const f32x4*>(base + off_d + R * t);
    return v;
  };
  auto store_tile = [&](float* base, int t, const f32x4& v) {
    if (real_d(t)) *reinterpret_cast<f32x4*>(base + off_d + R * t) = v;
  };
  auto store_hidden = [&](float* base, int th, const f32x4& v) {
    if (real_h(th)) *reinterpret_cast<f32x4*>(base + off_h + R * th) = v;
  };

  // (KL: no per-row accumulators -- with lam, y, f and act'(z) they do not fit 256 registers at d = hidden = 128 -- but sums
  //  over the wave's 16 rows in LDS, as the adjoint kernel keeps them)
  f32x4 lam[TD];
  [[maybe_unused]] f32x4 acc_rate[KL ? 1 : TD], acc_shift[KL ? 1 : TD];
#pragma unroll
  for (int t = 0; t < TD; ++t) {
    lam[t] = load_tile(p.lam, t);
    if constexpr (!KL) {
      acc_rate[t] = {0.0f, 0.0f, 0.0f, 0.0f};
      acc_shift[t] = {0.0f, 0.0f, 0.0f, 0.0f};
    }
  }

  // y_k is loaded one step ahead (issued before the last product of the previous step, which does not read it): a
  // load consumed right behind its issue would expose the memory latency once per step -- and per tile in the diffusion
  // terms, which use the same registers again instead of re-reading.
  f32x4 y[TD];
#pragma unroll
  for (int t = 0; t < TD; ++t) y[t] = load_tile(p.ys_all + (int64_t)(p.k_hi - 1 - p.ys_first) * p.B * dT, t);
  int jg = p.grad_last;
  for (int k = p.k_hi - 1; k >= p.k_lo; --k) {
    const float* srow = p.rows + (int64_t)k * 8;
    const float dt = srow[0], sw = srow[4];
    const uint32_t cell = p.cells[k];
    const int64_t slot = k - p.k_lo;
    const bool arrives = jg >= 0 && p.grad_step[jg] == k + 1;     // an output sits on boundary k + 1 (WEIGHTED: in step k)

    if constexpr (!WEIGHTED) {
#pragma unroll
      for (int t = 0; t < TD; ++t) {
        if (arrives) lam[t] += load_tile(p.grad_ys + (int64_t)jg * p.B * dT, t);
        if constexpr (!KL) store_tile(p.stash_lam + slot * p.B * dT, t, lam[t] * dt);     // (KL: once f is known, below)
      }
      if constexpr (KL) {
        if (arrives) al += p.grad_logqp[(int64_t)jg * p.B + row];
      }
      if (arrives) --jg;
    } else {
      // outputs jg, jg - 1, ... sit in step k: on boundary k + 1, or inside the step as w0 y_k + w1 y_{k+1} (base_solver.py:147,
      // interp.py:15-18) -- their w1 share joins lam = dL/dy_{k+1} here, their w0 share dL/dy_k at the end of the iteration
      if (arrives) {
        do {
          const float* gy = p.grad_ys + (int64_t)jg * p.B * dT;
          const float w0 = p.grad_w[2 * jg], w1 = p.grad_w[2 * jg + 1];
          if (w0 == 0.0f && w1 == 1.0f) {                              // on the boundary: the cotangent as it is
#pragma unroll
            for (int t = 0; t < TD; ++t) lam[t] += load_tile(gy, t);
            if constexpr (KL) al += p.grad_logqp[(int64_t)jg * p.B + row];
          } else {
#pragma unroll
            for (int t = 0; t < TD; ++t) lam[t] += load_tile(gy, t) * w1;
            if constexpr (KL) al += p.grad_logqp[(int64_t)jg * p.B + row] * w1;
          }
          --jg;
        } while (jg >= 0 && p.grad_step[jg] == k + 1);
      }
      if constexpr (!KL) {
#pragma unroll
        for (int t = 0; t < TD; ++t) store_tile(p.stash_lam + slot * p.B * dT, t, lam[t] * dt);
      }
    }
    __builtin_amdgcn_sched_barrier(0);

    // ---- hidden layer: z^T = W1^T y^T; keep act'(z), stash act(z) ---------------------------------------------------
    // (KL: f^T += W2^T act(z)^T as each tile of act(z) completes)
    f32x4 hid[TH];
    [[maybe_unused]] f32x4 f[KL ? TD : 1];
    if constexpr (KL) {
#pragma unroll
      for (int t = 0; t < TD; ++t) f[t] = {0.0f, 0.0f, 0.0f, 0.0f};
    }
#pragma unroll
    for (int th = 0; th < TH; ++th) {
      f32x4 z = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int t = 0; t < TD; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) z = TL::mfma(W1s[(R * t + 4 * part + r) * S1 + R * th + n], y[t][r], z);
      }
      // the A operands arrive as 2 TD two-address reads (ds_read2_b32: rows r, r+1 of W1s), each feeding two MFMAs: keep
      // four of them in flight ahead of the MFMAs instead of hipcc's read -> wait -> two MFMAs
      reads_ahead<2 * TD, 2>();
      f32x4 value;
      const f32x4 bias = lds_quad(b1s, R * th + 4 * part);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v, slope;
        activate_with_slope<ACT>(z[r] + bias[r], v, slope);
        value[r] = v;
        hid[th][r] = slope;
      }
      store_hidden(p.stash_hid + slot * p.B * hT, th, value);
      if constexpr (KL) {
        // (padded hidden units: act(0 + 0) is not 0 for softplus, but their W2 rows are zero in LDS)
#pragma unroll
        for (int t = 0; t < TD; ++t) {
#pragma unroll
          for (int r = 0; r < 4; ++r) f[t] = TL::mfma(W2s[(R * th + 4 * part + r) * S2 + R * t + n], value[r], f[t]);
        }
        reads_ahead<2 * TD, 2>();
      }
      __builtin_amdgcn_sched_barrier(0);
    }

    // ---- KL: the whole elementwise phase, ahead of the W2 product: w from f, the operand lam + w of that product (it takes
    //      f's registers), dt (lam + w) to the stash, then the diffusion terms and the column's own on lam and the sums ------
    if constexpr (KL) {
      constexpr bool kSigmoid = KIND == kKlEulerSigmoid;
#pragma unroll
      for (int t = 0; t < TD; ++t) {
        const int ch = R * t + 4 * part;
        float zn[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        uint64_t elem = elem0_lane + R * t;
        asm volatile("" : "+v"(elem));            // (keeps the step-invariant first Philox round inside the sweep)
        if (real_d(t)) normal4_straddle<float>(key, elem, cell, 0, kStreamW, zn);
        const f32x4 yt = y[t];
        const f32x4 cq = lds_quad(cs, ch), eq = lds_quad(es, ch), bq = lds_quad(b2s, ch);
        const f32x4 hrq = lds_quad(hrs, ch), hsq = lds_quad(hss, ch);
        float rate_terms[4], shift_terms[4], hrate_terms[4], hshift_terms[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float yy = yt[r], cc = cq[r], l = lam[t][r];
          const DiffusionValue dv = diffusion_value(kSigmoid, p.diff_amp, cc, eq[r], yy);
          const KlShare kl = kl_share(f[t][r] + bq[r], hrq[r] * yy + hsq[r], dv.g, al, dt, real_d(t));
          f[t][r] = real_d(t) ? l + kl.w : l;
          const float kqq = kl.kq * dv.q;                              // a_l dt (u^2 / safe) dg/de
          const float w = zn[r] * sw;
          float to_shift, to_rate, step;
          if constexpr (KIND != kKlMilsteinAffine) {
            const float lw = (l * w) * dv.q;
            to_shift = lw;
            to_rate = lw * yy;
            step = lw * cc;
          } else {
            const float v = milstein_v<float>(w, dt, 0.5f, true);         // (the KL column is carried for Ito SDEs only)
            const float cy = cc * yy;
            to_shift = l * (w + cc * v);
            to_rate = l * (yy * w + v * ((cy + eq[r]) + cy));
            step = l * (cc * w + (cc * cc) * v);
          }
          shift_terms[r] = row_total((to_shift - kqq) * own_row);
          rate_terms[r] = row_total((to_rate - kqq * yy) * own_row);
          hshift_terms[r] = row_total(-kl.dtw * own_row);
          hrate_terms[r] = row_total(-(kl.dtw * yy) * own_row);
          lam[t][r] = l + (step - (hrq[r] * kl.dtw + kqq * cc));
          asm volatile("" : "+v"(lam[t][r]), "+v"(f[t][r]));     // (materialised here, as in the adjoint kernel)
        }
        store_tile(p.stash_lam + slot * p.B * dT, t, f[t] * dt);
        // summed over the 16 rows of the wave (the 16 lanes of a DPP row hold one channel quad of 16 rows); the row's last
        // lane adds the totals to the wave's LDS accumulators (ds_add_f32: one lane per address, in order per wave)
        if (n == R - 1 && real_d(t)) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            atomicAdd(&wave_sums[ch + r], rate_terms[r]);
            atomicAdd(&wave_sums[D + ch + r], shift_terms[r]);
            atomicAdd(&wave_sums[2 * D + ch + r], hrate_terms[r]);
            atomicAdd(&wave_sums[3 * D + ch + r], hshift_terms[r]);
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }

    // ---- u^T = W2 lam^T (rows of W2s, four consecutive channels per lane); delta = u * act'(z) * dt ----------------
    // (KL: W2 (lam + w)^T)
#pragma unroll
    for (int th = 0; th < TH; ++th) {
      f32x4 u = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int t = 0; t < TD; ++t) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(&W2s[(R * th + n) * S2 + R * t + 4 * part]);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if constexpr (KL) u = TL::mfma(a[r], f[t][r], u);
          else u = TL::mfma(a[r], lam[t][r], u);
        }
        if ((t + 1) % 4 == 0) __builtin_amdgcn_sched_barrier(0);
      }
      hid[th] = (u * hid[th]) * dt;
      store_hidden(p.stash_delta + slot * p.B * hT, th, hid[th]);
      __builtin_amdgcn_sched_barrier(0);
    }

    // ---- diffusion: dW_k again from the counter RNG; lam <- lam + lam c dW ------------------------------------------
    if constexpr (!KL) {
#pragma unroll
    for (int t = 0; t < TD; ++t) {
      const int ch = R * t + 4 * part;
      float zn[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      // (opaque to the optimiser: otherwise the step-invariant first Philox round of every tile is hoisted out of the
      //  sweep and pinned in ~4 registers per tile)
      uint64_t quad = quad0 + 4 * t;
      asm volatile("" : "+v"(quad));
      if (real_d(t)) normal4_pairs<float>(key, quad, cell, 0, kStreamW, zn);
      const f32x4 yt = y[t];
      const f32x4 cq = lds_quad(cs, ch);
      const f32x4 eq = lds_quad(es, ch);
      if (p.method == TSDE_TRAJ_EULER) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          // dg/de = q, dg/dc = q y, dg/dy = q c   (affine: q = 1)
          const float q = diffusion_value(p.diff_kind == TSDE_DIFF_SIGMOID, p.diff_amp, cq[r], eq[r], yt[r]).q;
          const float lw = (lam[t][r] * (zn[r] * sw)) * q;
          acc_shift[t][r] += lw;
          acc_rate[t][r] += lw * yt[r];
          lam[t][r] += lw * cq[r];
        }
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float w = zn[r] * sw, cc = cq[r];
          const float v = milstein_v<float>(w, dt, 0.5f, p.method == TSDE_TRAJ_MILSTEIN_ITO);
          const float cy = cc * yt[r];
          const float l = lam[t][r];
          acc_shift[t][r] += l * (w + cc * v);
          acc_rate[t][r] += l * (yt[r] * w + v * ((cy + eq[r]) + cy));
          lam[t][r] += l * (cc * w + (cc * cc) * v);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    }

    if (k > p.k_lo) {
#pragma unroll
      for (int t = 0; t < TD; ++t) y[t] = load_tile(p.ys_all + (int64_t)(k - 1 - p.ys_first) * p.B * dT, t);
    }
    __builtin_amdgcn_sched_barrier(0);

    // ---- lam^T += W1 delta^T (rows of W1s, four consecutive hidden units per lane) ------------------------------------
#pragma unroll
    for (int t = 0; t < TD; ++t) {
      f32x4 back = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int th = 0; th < TH; ++th) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(&W1s[(R * t + n) * S1 + R * th + 4 * part]);
#pragma unroll
        for (int r = 0; r < 4; ++r) back = TL::mfma(a[r], hid[th][r], back);
        if ((th + 1) % 4 == 0) __builtin_amdgcn_sched_barrier(0);
      }
      lam[t] += back;
      __builtin_amdgcn_sched_barrier(0);
    }

    // ---- lam is dL/dy_k: the w0 share of the outputs inside this step (a_l: from step k - 1 down). They are the outputs
    //      above jg again, found from the table: nothing of them is kept across the step -------------------------------------
    if constexpr (WEIGHTED) {
      for (int j = jg + 1; j <= p.grad_last && p.grad_step[j] == k + 1; ++j) {
        const float w0 = p.grad_w[2 * j];
        if (w0 == 0.0f) continue;
        const float* gy = p.grad_ys + (int64_t)j * p.B * dT;
#pragma unroll
        for (int t = 0; t < TD; ++t) lam[t] += load_tile(gy, t) * w0;
        if constexpr (KL) al += p.grad_logqp[(int64_t)j * p.B + row] * w0;
      }
    }
  }

#pragma unroll
  for (int t = 0; t < TD; ++t) {
    store_tile(p.lam, t, lam[t]);
    if constexpr (!KL) {
      store_tile(p.row_rate, t, load_tile(p.row_rate, t) + acc_rate[t]);
      store_tile(p.row_shift, t, load_tile(p.row_shift, t) + acc_shift[t]);
    }
  }
  if constexpr (KL) {
    if (part == 0) p.a_l[row] = al;
    // the wave's sums join row `row0` of the four (B, d) arrays
    for (int i = lane; i < dT; i += 64) {
      p.row_rate[row0 * dT + i] += wave_sums[i];
      p.row_shift[row0 * dT + i] += wave_sums[D + i];
      p.row_hrate[row0 * dT + i] += wave_sums[2 * D + i];
      p.row_hshift[row0 * dT + i] += wave_sums[3 * D + i];
    }
  }
}

// 8-wave blocks (two waves per SIMD, 256 registers each) everywhere except the padded 128-channel case, whose bounds
// tests push the sweep past 256 registers: 4-wave blocks there (one wave per SIMD, 512 registers) instead of spilling.
struct MlpBackwardPolicy {
  template <int D, int H, int ACT, bool FULL>
  static hipError_t launch(const MlpBackArgs& p, hipStream_t s) {
    constexpr int NW = (!FULL && D == 128) ? 4 : 8;
    if (p.grad_w != nullptr)
      return launch_rows_per_wave<mlp_backward_kernel<D, H, ACT, NW, FULL, false, 0, true>, NW, 16>(
          p, MlpLds<16>::bytes(D, H, 2), s);
    return launch_rows_per_wave<mlp_backward_kernel<D, H, ACT, NW, FULL>, NW, 16>(p, MlpLds<16>::bytes(D, H, 2), s);
  }
};

// The KL instantiation. With per-row register accumulators for its four sums (7 D/4 + H/4 live registers per lane) the
// d = hidden = 128 shape spilled 470 dwords as an 8-wave block and still 28 as a 4-wave block; with the sums in LDS (lam, y,
// f / lam + w and act'(z): 3 D/4 + H/4) and one elementwise phase per instantiation (KIND) every shape runs as 8-wave blocks
// without a spilled vector register and without scratch (profiles/logqp_backprop_resource_usage_new.txt: 235 registers at
// d = hidden = 128).
struct MlpBackwardKlPolicy {
  template <int D, int H, int ACT, bool FULL>
  static hipError_t launch(const MlpBackKlArgs& p, hipStream_t s) {
    constexpr int NW = 8;
    constexpr size_t lds_bytes = MlpLds<16>::bytes(D, H, 5, NW * 4 * D);
    return p.grad_w != nullptr ? launch_kind<D, H, ACT, FULL, true>(p, lds_bytes, s)
                               : launch_kind<D, H, ACT, FULL, false>(p, lds_bytes, s);
  }
  template <int D, int H, int ACT, bool FULL, bool WEIGHTED>
  static hipError_t launch_kind(const MlpBackKlArgs& p, size_t lds_bytes, hipStream_t s) {
    constexpr int NW = 8;
    if (p.method != TSDE_TRAJ_EULER)
      return launch_rows_per_wave<mlp_backward_kernel<D, H, ACT, NW, FULL, true, kKlMilsteinAffine, WEIGHTED>, NW, 16>(
          p, lds_bytes, s);
    if (p.diff_kind == TSDE_DIFF_SIGMOID)
      return launch_rows_per_wave<mlp_backward_kernel<D, H, ACT, NW, FULL, true, kKlEulerSigmoid, WEIGHTED>, NW, 16>(
          p, lds_bytes, s);
    return launch_rows_per_wave<mlp_backward_kernel<D, H, ACT, NW, FULL, true, kKlEulerAffine, WEIGHTED>, NW, 16>(
        p, lds_bytes, s);
  }
};

static void fill_back_args(MlpBackArgs& p, void* lam, void* stash_lam, void* stash_hid, void* stash_delta, void* row_rate,
                           void* row_shift, const void* ys_all, int32_t ys_first, const void* grad_ys,
                           const int32_t* grad_step, const void* grad_w, int32_t grad_last, int64_t rows, int64_t d, int64_t h,
                           const void* W1, const void* b1, const void* W2, const void* c, const void* e, int diff_kind,
                           double diff_amp, int method, const tsde_traj_t* tr, int32_t k_lo, int32_t k_hi, NoiseKey key,
                           const uint64_t* key_dev) {
  fill_mlp_core(p, rows, d, h, W1, b1, W2, c, e, diff_kind, diff_amp, tr, key, key_dev);
  p.lam = (float*)lam;
  p.stash_lam = (float*)stash_lam;
  p.stash_hid = (float*)stash_hid;
  p.stash_delta = (float*)stash_delta;
  p.row_rate = (float*)row_rate;
  p.row_shift = (float*)row_shift;
  p.ys_all = (const float*)ys_all;
  p.ys_first = ys_first;
  p.grad_ys = (const float*)grad_ys;
  p.grad_step = grad_step;
  p.grad_w = (const float*)grad_w;
  p.grad_last = grad_last;
  p.method = method;
  p.k_lo = k_lo;
  p.k_hi = k_hi;
}

hipError_t launch_trajectory_mlp_diag_backward(void* lam, void* stash_lam, void* stash_hid, void* stash_delta,
                                               void* row_rate, void* row_shift, const void* ys_all,
                                               int32_t ys_first, const void* grad_ys, const int32_t* grad_step,
                                               const void* grad_w, int32_t grad_last,
                                               int64_t rows, int64_t d, int64_t h, const void* W1, const void* b1,
                                               const void* W2, const void* c, const void* e, int diff_kind,
                                               double diff_amp, int act, int method, const tsde_traj_t* tr,
                                               int32_t k_lo, int32_t k_hi, NoiseKey key, const uint64_t* key_dev,
                                               hipStream_t s) {
  MlpBackArgs p;
  fill_back_args(p, lam, stash_lam, stash_hid, stash_delta, row_rate, row_shift, ys_all, ys_first, grad_ys, grad_step,
                 grad_w, grad_last, rows, d, h, W1, b1, W2, c, e, diff_kind, diff_amp, method, tr, k_lo, k_hi, key, key_dev);
  if (rows <= 0 || k_hi <= k_lo) return hipSuccess;
  return mlp_ladder<MlpBackwardPolicy>(p, act, s);
}

hipError_t launch_trajectory_mlp_diag_logqp_backward(void* lam, void* a_l, void* stash_lam, void* stash_hid,
                                                     void* stash_delta, void* row_rate, void* row_shift, void* row_hrate,
                                                     void* row_hshift, const void* ys_all, int32_t ys_first,
                                                     const void* grad_ys, const void* grad_logqp, const int32_t* grad_step,
                                                     const void* grad_w, int32_t grad_last, int64_t rows, int64_t d, int64_t h,
                                                     const void* W1, const void* b1, const void* W2, const void* b2, const void* c,
                                                     const void* e, const void* hr, const void* hs, int diff_kind,
                                                     double diff_amp, int act, int method, const tsde_traj_t* tr,
                                                     int32_t k_lo, int32_t k_hi, int64_t bm_stride, NoiseKey key,
                                                     const uint64_t* key_dev, hipStream_t s) {
  MlpBackKlArgs p;
  fill_back_args(p, lam, stash_lam, stash_hid, stash_delta, row_rate, row_shift, ys_all, ys_first, grad_ys, grad_step,
                 grad_w, grad_last, rows, d, h, W1, b1, W2, c, e, diff_kind, diff_amp, method, tr, k_lo, k_hi, key, key_dev);
  p.a_l = (float*)a_l;
  p.grad_logqp = (const float*)grad_logqp;
  p.b2 = (const float*)b2;
  p.hr = (const float*)hr;
  p.hs = (const float*)hs;
  p.row_hrate = (float*)row_hrate;
  p.row_hshift = (float*)row_hshift;
  p.bm_stride = bm_stride;
  if (rows <= 0 || k_hi <= k_lo) return hipSuccess;
  return mlp_ladder<MlpBackwardKlPolicy>(p, act, s);
}

// ---- C = A^T B (and the column sums of A) over a tall K --------------------------------------------------------------
// A block owns a contiguous K range and walks it in tiles of 32 rows: 16-byte coalesced loads of both operands into
// registers (the NEXT tile's loads are in flight while the current one is multiplied), one LDS copy per tile, double
// buffered (one barrier per tile). Waves are arranged 4 (along M) x 2 (along N); a wave holds MT x NT accumulator tiles
// of 16 x 16 and reads its operands from LDS in MFMA layout:
//   A operand of v_mfma_f32_16x16x4_f32: lane l supplies A^T[i = l % 16][k = l / 16] = tile[k0 + l / 16][16 ti + l % 16]
//   B operand:                           lane l supplies B[k = l / 16][j = l % 16]   = tile[k0 + l / 16][16 tj + l % 16]
// (row stride padded by 16 floats: the two K rows of a half-wave then sit in opposite halves of the 32 banks).
// The loader's threads keep fixed columns, so the column sums of A (the bias gradients) cost one add per loaded value.
constexpr int kGramRows = 32;

template <int MT, int NT, bool VEC>
__global__ void __launch_bounds__(512) gram_kernel(float* __restrict__ partials, float* __restrict__ colsums,
                                                   const float* __restrict__ A, int64_t lda,
                                                   const float* __restrict__ Bm, int64_t ldb, int64_t K, int32_t M,
                                                   int32_t N, int64_t rows_per_block) {
  using TL = Tile<16>;
  constexpr int MP = 64 * MT, NP = 32 * NT;                 // padded widths
  constexpr int SA = MP + 16, SB = NP + 16;                 // LDS row strides (floats)
  constexpr int QA = MP / 4, QB = NP / 4;                   // 16-byte slots per tile row
  constexpr int LA = (kGramRows * QA + 511) / 512, LB = (kGramRows * QB + 511) / 512;   // slots per thread
  __shared__ float As[2][kGramRows * SA];
  __shared__ float Bs[2][kGramRows * SB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int part = lane >> 4, n = lane & 15;
  const int wm = wave & 3, wn = wave >> 2;

  f32x4 acc[MT][NT];
#pragma unroll
  for (int a = 0; a < MT; ++a)
#pragma unroll
    for (int b = 0; b < NT; ++b) acc[a][b] = {0.0f, 0.0f, 0.0f, 0.0f};
  f32x4 csum = {0.0f, 0.0f, 0.0f, 0.0f};                    // columns 4 (tid % QA) .. + 3 of A, this thread's rows

  const int64_t k0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t k1 = k0 + rows_per_block < K ? k0 + rows_per_block : K;
  const int ntiles = k1 > k0 ? (int)((k1 - k0 + kGramRows - 1) / kGramRows) : 0;

  // Loader: a slot is 16 bytes of one tile row. `fetch` only ISSUES the load (from a clamped, always valid address);
  // whether the slot lies inside the tile is applied when the registers are copied to LDS, one tile of matrix
  // instructions later -- anything that touches the loaded value earlier (a select, the column sum) would put the
  // wait for the load in front of those instructions.
  f32x4 ra[LA], rb[LB];
  bool in_a[LA], in_b[LB];
  auto fetch = [&](const float* __restrict__ src, int64_t ld, int32_t width, int q_per_row, int slot, int64_t kk,
                   bool& inside) {
    const int r = slot / q_per_row, c = 4 * (slot % q_per_row);
    const int64_t krow = kk + r;
    inside = r < kGramRows && krow < k1 && c < width;
    if constexpr (VEC) {
      const int64_t row_c = krow < K ? krow : K - 1;        // (k1 > k0 >= 0 here: K - 1 is a valid row)
      const int col_c = c < width ? c : width - 4;
      return *reinterpret_cast<const f32x4*>(src + row_c * ld + col_c);
    } else {
      f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
      if (inside) {
        const float* q = src + krow * ld + c;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (c + e < width) v[e] = q[e];
      }
      return v;
    }
  };
  auto load_tile = [&](int tile) {
    const int64_t kk = k0 + (int64_t)tile * kGramRows;
#pragma unroll
    for (int i = 0; i < LA; ++i) ra[i] = fetch(A, lda, M, QA, tid + 512 * i, kk, in_a[i]);
#pragma unroll
    for (int i = 0; i < LB; ++i) rb[i] = fetch(Bm, ldb, N, QB, tid + 512 * i, kk, in_b[i]);
  };
  auto stage_tile = [&](int buf) {
    const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int i = 0; i < LA; ++i) {
      const int slot = tid + 512 * i;
      const f32x4 v = in_a[i] ? ra[i] : zero;
      if (slot < kGramRows * QA) *reinterpret_cast<f32x4*>(&As[buf][(slot / QA) * SA + 4 * (slot % QA)]) = v;
      csum += v;
    }
#pragma unroll
    for (int i = 0; i < LB; ++i) {
      const int slot = tid + 512 * i;
      const f32x4 v = in_b[i] ? rb[i] : zero;
      if (slot < kGramRows * QB) *reinterpret_cast<f32x4*>(&Bs[buf][(slot / QB) * SB + 4 * (slot % QB)]) = v;
    }
  };

  if (ntiles > 0) {
    load_tile(0);
    stage_tile(0);
  }
  __syncthreads();
  for (int tile = 0; tile < ntiles; ++tile) {
    const int buf = tile & 1;
    if (tile + 1 < ntiles) load_tile(tile + 1);
#pragma unroll
    for (int g = 0; g < kGramRows / 4; ++g) {
      float fa[MT], fb[NT];
#pragma unroll
      for (int a = 0; a < MT; ++a) fa[a] = As[buf][(4 * g + part) * SA + 16 * (wm * MT + a) + n];
#pragma unroll
      for (int b = 0; b < NT; ++b) fb[b] = Bs[buf][(4 * g + part) * SB + 16 * (wn * NT + b) + n];
#pragma unroll
      for (int a = 0; a < MT; ++a)
#pragma unroll
        for (int b = 0; b < NT; ++b) acc[a][b] = TL::mfma(fa[a], fb[b], acc[a][b]);
    }
    if (tile + 1 < ntiles) stage_tile(buf ^ 1);
    __syncthreads();
  }

  float* out = partials + (int64_t)blockIdx.x * M * N;
#pragma unroll
  for (int a = 0; a < MT; ++a)
#pragma unroll
    for (int b = 0; b < NT; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 16 * (wm * MT + a) + 4 * part + r, j = 16 * (wn * NT + b) + n;
        if (i < M && j < N) out[(int64_t)i * N + j] = acc[a][b][r];
      }

  if (colsums != nullptr) {
    // thread tid summed columns 4 (tid % QA) ..+3 over its rows: 512 / QA threads per column quad, added up in a
    // fixed order through LDS (the tile buffers are free now: the loop ended on a barrier)
    float* scratch = &As[0][0];                             // (512 / QA) x MP floats <= 2 * 32 * SA
    *reinterpret_cast<f32x4*>(&scratch[(tid / QA) * MP + 4 * (tid % QA)]) = csum;
    __syncthreads();
    if (tid < M) {
      float total = 0.0f;
      for (int j = 0; j < 512 / QA; ++j) total += scratch[j * MP + tid];
      colsums[(int64_t)blockIdx.x * M + tid] = total;
    }
  }
}

template <int MT, int NT>
static hipError_t launch_gram_vec(float* partials, float* colsums, const float* A, int64_t lda, const float* Bm,
                                  int64_t ldb, int64_t K, int32_t M, int32_t N, int32_t blocks, int64_t rows_per_block,
                                  hipStream_t s) {
  const bool vec = M % 4 == 0 && N % 4 == 0 && lda % 4 == 0 && ldb % 4 == 0 &&
                   ((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(Bm)) & 15u) == 0;
  if (vec)
    hipLaunchKernelGGL((gram_kernel<MT, NT, true>), dim3(blocks), dim3(512), 0, s, partials, colsums, A, lda, Bm, ldb, K,
                       M, N, rows_per_block);
  else
    hipLaunchKernelGGL((gram_kernel<MT, NT, false>), dim3(blocks), dim3(512), 0, s, partials, colsums, A, lda, Bm, ldb,
                       K, M, N, rows_per_block);
  return hipGetLastError();
}

template <int MT>
static hipError_t launch_gram_n(float* partials, float* colsums, const float* A, int64_t lda, const float* Bm,
                                int64_t ldb, int64_t K, int32_t M, int32_t N, int32_t blocks, int64_t rows_per_block,
                                hipStream_t s) {
  if (N <= 32) return launch_gram_vec<MT, 1>(partials, colsums, A, lda, Bm, ldb, K, M, N, blocks, rows_per_block, s);
  if (N <= 64) return launch_gram_vec<MT, 2>(partials, colsums, A, lda, Bm, ldb, K, M, N, blocks, rows_per_block, s);
  if (N <= 128) return launch_gram_vec<MT, 4>(partials, colsums, A, lda, Bm, ldb, K, M, N, blocks, rows_per_block, s);
  return hipErrorInvalidValue;
}

hipError_t launch_gram_partials(void* partials, void* colsums, const void* A, int64_t lda, const void* Bm, int64_t ldb,
                                int64_t K, int64_t M, int64_t N, int32_t blocks, hipStream_t s) {
  if (K <= 0 || M <= 0 || N <= 0 || blocks <= 0) return hipErrorInvalidValue;
  int64_t rows_per_block = (K + blocks - 1) / blocks;
  rows_per_block = (rows_per_block + kGramRows - 1) / kGramRows * kGramRows;       // whole tiles
  if (M <= 64)
    return launch_gram_n<1>((float*)partials, (float*)colsums, (const float*)A, lda, (const float*)Bm, ldb, K,
                            (int32_t)M, (int32_t)N, blocks, rows_per_block, s);
  if (M <= 128)
    return launch_gram_n<2>((float*)partials, (float*)colsums, (const float*)A, lda, (const float*)Bm, ldb, K,
                            (int32_t)M, (int32_t)N, blocks, rows_per_block, s);
  return hipErrorInvalidValue;
}

}  // namespace tsde
