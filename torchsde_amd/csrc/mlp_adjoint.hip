// The stochastic adjoint of the perceptron-drift SDE (closed_form.py: MLPDriftDiagonalSDE) on the matrix cores:
// `sdeint_adjoint(..., adjoint_method="euler")` for that module as ONE kernel per chunk of steps instead of the
// reference's ~60 torch kernels per step (adjoint.py:64-127 driving adjoint_sde.py:177-230, 296-323 through
// methods/euler.py:29-37).
//
// The reference integrates, backwards in time and on the same Brownian path, the augmented state (y, a, a_theta):
//
//   f~ = f - g g'            (Ito; the double Stratonovich correction of adjoint_sde.py:177-216. Stratonovich: f~ = f)
//   y      <- y - f~ dt - g dW                                     (the forward state, RECONSTRUCTED, not stored)
//   a      <- a + dt J_f^T a + a (g' dW - dt g g'')                (the g'^2 terms of the correction cancel)
//   a_th_f <- a_th_f + dt a^T df/dtheta_f                          (perceptron weights and biases)
//   a_th_g <- a_th_g + a (dW dg/dtheta_g - dt g dg'/dtheta_g)      (diffusion rate c and shift e; Stratonovich: first term)
//
// and with `adjoint_method="milstein"` (methods/milstein.py:52-74 on adjoint_sde.py:332-377; the default for diagonal
// Ito noise) the step gains, with v = (dW^2 - dt) / 2 (Ito) or dW^2 / 2 (Stratonovich), the ELEMENTWISE terms
//
//   y      <- ... + v g g'            a <- ... + a v (g'^2 - g g'')
//   a_th_g <- ... + a v (g' dg/dtheta_g - g dg'/dtheta_g)
//
// (g is diagonal: Milstein's correction never touches the perceptron, so the matrix products are Euler's)
//
// everything evaluated at the current reconstructed y, dW the increment of the forward cell the step walks back over.
// With f = W2^T act(W1^T y + b1) + b2 that is four matrix products per step, on v_mfma_f32_16x16x4_f32 against the
// same two LDS weight arrays the sampling and reverse-sweep kernels use (mlp_trajectory.hip, mlp_backward.hip):
//
//   z = W1^T y          (as stored)          -> h = act(z), act'(z)
//   f = W2^T h          (as stored)          accumulated tile by tile as the h tiles complete
//   u = W2 a            (16-byte rows)       -> delta = u * act'(z) * dt
//   a += W1 delta       (16-byte rows)
//
// A wave owns 16 batch rows for all steps of the launch; y and a stay in registers in the MFMA accumulator layout; dW is
// regenerated from the counter RNG; the per-step factors of the weight gradients (dt a, h, delta, y) go to a stash in
// HBM for tsde_gram_partials (mlp_backward.hip); the diffusion-parameter terms are summed over the wave's 16 rows with
// DPP row shifts and accumulated per wave in LDS. Memory is O(chunk),
// independent of the number of steps: nothing of the forward pass is kept but the states at the output times.
#include <type_traits>

#include "tsde_common.h"
#include "tsde_launch.h"
#include "tsde_mlp.h"

namespace tsde {

struct MlpAdjArgs {
  float* y;                 // (B, d)  in: state at boundary k_hi; out: reconstructed state at k_lo
  float* a;                 // (B, d)  in: dL/dy at boundary k_hi; out: at k_lo
  float* stash_a;           // (k_hi - k_lo, B, d)   dt_k * a
  float* stash_hid;         // (k_hi - k_lo, B, h)   act(W1^T y + b1)
  float* stash_delta;       // (k_hi - k_lo, B, h)   delta
  float* stash_y;           // (k_hi - k_lo, B, d)   the y the step was evaluated at
  float* row_rate;          // (B, d)  row 16 k += the sums of rows 16 k .. 16 k + 15 for dL/dc (the caller sums over the batch)
  float* row_shift;         // (B, d)  ... for dL/de
  const float* W1;          // (d, h) input-major, as MlpArgs
  const float* b1;          // (h)
  const float* W2;          // (h, d)
  const float* b2;          // (d)
  const float *c, *e;       // (d) diffusion coefficients
  int32_t diff_kind;        // TSDE_DIFF_AFFINE / TSDE_DIFF_SIGMOID
  float diff_amp;
  int32_t ito;              // bit 0: Ito (corrected drift) / Stratonovich; bit 1: Milstein backward step / Euler
  const float* rows;        // (n_steps, 8) schedule rows of the FORWARD cells: [0] = dt, [4] = sqrt(h)
  const uint32_t* cells;
  int64_t B;
  int32_t d, h;
  int32_t k_lo, k_hi;
  NoiseKey key;
  const uint64_t* key_dev;
};

// The KL instantiation (`sdeint_adjoint(..., logqp=True)` with a per-channel affine prior drift h = hr * y + hs): the forward
// solve carried the column l, l' = f_l = 0.5 sum_i u_i^2, u = (f - h) / safe(g) (base_sde.py:240-306). Its cotangent a_l
// is constant between outputs (nothing depends on l) and reaches the rest of the adjoint through d f_l / d(y, theta): with
// w = a_l u / safe (per channel)
//
//   the drift network sees the cotangent a + w instead of a     (u^T = W2 (a + w)^T; the stash holds dt (a + w))
//   a      <- ... + dt (-hr w - a_l u^2 g' / safe)
//   a_th_g <- ... - a_l dt (u^2 / safe) dg/dtheta_g            (no such term where the divisor is clamped)
//   a_hr   <- a_hr - dt w y        a_hs <- a_hs - dt w          (the prior's coefficients)
//
// The column's diffusion is 0: the Ito correction and the Milstein terms of the step are unchanged.
struct MlpAdjKlArgs : MlpAdjArgs {
  const float* a_l;         // (B) cotangent of the column l, unchanged by the launch
  const float *hr, *hs;     // (d) prior drift coefficients
  float* row_hrate;         // (B, d) as row_rate, for dL/dhr
  float* row_hshift;        // (B, d) ... for dL/dhs
  int64_t bm_stride;        // row stride of the Brownian field: d + 1
};

// The kernel's LDS behind b2 / c / e (MlpLds): kAdjSums x D sums per wave -- rate, shift; KL: the prior's (hr, hs) after
// them -- and, KL, hr and hs themselves.
template <bool KL>
constexpr int kAdjSums = KL ? 4 : 2;
template <int D, int NW, bool KL>
constexpr int kAdjExtraFloats = NW * kAdjSums<KL> * D + (KL ? 2 * D : 0);

template <int D, int H, int ACT, int NW, bool FULL, bool MILSTEIN, bool KL = false>
__global__ void __launch_bounds__(NW * 64)
    mlp_adjoint_kernel(const std::conditional_t<KL, MlpAdjKlArgs, MlpAdjArgs> p) {
  constexpr int R = 16, kSums = kAdjSums<KL>;
  using TL = Tile<R>;
  constexpr int TD = D / R, TH = H / R, kThreads = NW * 64;
  using L = MlpLds<R>;
  constexpr int S1 = H + L::kPad, S2 = D + L::kPad;
  extern __shared__ float lds[];
  float* W1s = lds;                         // D rows of S1: W1s[channel][hidden]
  float* W2s = lds + L::w2(D, H);           // H rows of S2: W2s[hidden][channel]
  float* b1s = lds + L::b1(D, H);           // H
  float* b2s = lds + L::vec(D, H, 0);       // D
  float* cs = lds + L::vec(D, H, 1);        // D
  float* es = lds + L::vec(D, H, 2);        // D
  float* sums = lds + L::vec(D, H, 3);      // NW x 2 x D: per wave, the diffusion-parameter sums (rate, shift) of its 16 rows
  //                                           (KL: NW x 4 x D, the prior's (hr, hs) after them, then hr and hs themselves)
  [[maybe_unused]] float* hrs = sums + NW * kSums * D;      // D
  [[maybe_unused]] float* hss = hrs + D;                    // D
  const int dT = p.d, hT = p.h;
  stage_perceptron<D, H, R, kThreads>(lds, p.W1, p.W2, p.b1, dT, hT);
  for (int i = threadIdx.x; i < D; i += kThreads) {
    b2s[i] = i < dT ? p.b2[i] : 0.0f;
    cs[i] = i < dT ? p.c[i] : 0.0f;
    es[i] = i < dT ? p.e[i] : 0.0f;
    if constexpr (KL) {
      hrs[i] = i < dT ? p.hr[i] : 0.0f;
      hss[i] = i < dT ? p.hs[i] : 0.0f;
    }
  }
  for (int i = threadIdx.x; i < NW * kSums * D; i += kThreads) sums[i] = 0.0f;
  __syncthreads();

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int part = lane / R, n = lane % R;
  // (as in the reverse sweep: a wave without rows is done; surplus lanes of the last partial wave shadow its last row)
  const int64_t row0 = ((int64_t)blockIdx.x * NW + wave) * R;
  if (row0 >= p.B) return;
  const int64_t row = row0 + n < p.B ? row0 + n : p.B - 1;
  const float own_row = row0 + n < p.B ? 1.0f : 0.0f;     // (a shadow lane of the last partial wave adds nothing to the sums)
  float* wave_sums = sums + wave * kSums * D;
  const NoiseKey key = launch_key(p.key, p.key_dev);
  const uint32_t off_d = (uint32_t)(row * dT) + 4 * part, off_h = (uint32_t)(row * hT) + 4 * part;
  const uint64_t quad0 = (key.elem0 + (uint64_t)(row * dT) + 4 * part) >> 2;
  // KL: the lane's first element of the field, quad-aligned on every fourth row only (normal4_straddle)
  [[maybe_unused]] uint64_t elem0_lane = 0;
  [[maybe_unused]] float al = 0.0f;
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

  f32x4 y[TD], a[TD];
#pragma unroll
  for (int t = 0; t < TD; ++t) {
    y[t] = load_tile(p.y, t);
    a[t] = load_tile(p.a, t);
  }
  const bool sigmoid = p.diff_kind == TSDE_DIFF_SIGMOID;
  const float ito = (p.ito & 1) ? 1.0f : 0.0f;

  for (int k = p.k_hi - 1; k >= p.k_lo; --k) {
    const float* srow = p.rows + (int64_t)k * 8;
    const float dt = srow[0], sw = srow[4];
    const uint32_t cell = p.cells[k];
    const int64_t slot = k - p.k_lo;

#pragma unroll
    for (int t = 0; t < TD; ++t) {
      if constexpr (!KL) store_tile(p.stash_a + slot * p.B * dT, t, a[t] * dt);     // (KL: once f is known, below)
      store_tile(p.stash_y + slot * p.B * dT, t, y[t]);
    }
    __builtin_amdgcn_sched_barrier(0);

    // ---- z^T = W1^T y^T -> h = act(z) (stashed), act'(z) (kept); f^T += W2^T h^T as each h tile completes ------------
    f32x4 hid[TH], f[TD];
#pragma unroll
    for (int t = 0; t < TD; ++t) f[t] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int th = 0; th < TH; ++th) {
      f32x4 z = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int t = 0; t < TD; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) z = TL::mfma(W1s[(R * t + 4 * part + r) * S1 + R * th + n], y[t][r], z);
      }
      // (as in the reverse sweep: the A operands arrive as 2 TD two-address reads, each feeding two MFMAs; keep four of
      //  them in flight ahead of the MFMAs instead of letting every read of the tile be hoisted to the top)
      __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
#pragma unroll
      for (int i = 0; i < 2 * TD; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
        if (i < 2 * TD - 4) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
      f32x4 value;
      const f32x4 bias = lds_quad(b1s, R * th + 4 * part);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v, slope;
        activate_with_slope<ACT>(z[r] + bias[r], v, slope);
        value[r] = v;
        hid[th][r] = slope;
      }
      // padded hidden units: act(0 + 0) is not 0 (softplus), but their W2 rows are zero in LDS, so they add nothing
      store_hidden(p.stash_hid + slot * p.B * hT, th, value);
#pragma unroll
      for (int t = 0; t < TD; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) f[t] = TL::mfma(W2s[(R * th + 4 * part + r) * S2 + R * t + n], value[r], f[t]);
      }
      __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
#pragma unroll
      for (int i = 0; i < 2 * TD; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
        if (i < 2 * TD - 4) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }

    // ---- KL: the cotangent the drift network sees, a + w with w = a_l u / safe; dt (a + w) to the stash ------------------
    [[maybe_unused]] f32x4 ap[KL ? TD : 1];
    if constexpr (KL) {
      auto cotangent = [&](auto is_sigmoid) {
        constexpr bool kSigmoid = decltype(is_sigmoid)::value;
#pragma unroll
        for (int t = 0; t < TD; ++t) {
          const int ch = R * t + 4 * part;
          const f32x4 cq = lds_quad(cs, ch), eq = lds_quad(es, ch), bq = lds_quad(b2s, ch);
          const f32x4 hrq = lds_quad(hrs, ch), hsq = lds_quad(hss, ch);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float yt = y[t][r];
            const float g = diffusion_value(kSigmoid, p.diff_amp, cq[r], eq[r], yt).g;
            const float wk = kl_cotangent(f[t][r] + bq[r], hrq[r] * yt + hsq[r], g, al);
            ap[t][r] = real_d(t) ? a[t][r] + wk : a[t][r];       // (a padded channel: g may be 0 there; no share)
          }
          store_tile(p.stash_a + slot * p.B * dT, t, ap[t] * dt);
          __builtin_amdgcn_sched_barrier(0);
        }
      };
      if (sigmoid) cotangent(std::true_type{});
      else cotangent(std::false_type{});
    }

    // ---- u^T = W2 a^T (rows of W2s, four consecutive channels per lane); delta = u * act'(z) * dt --------------------
#pragma unroll
    for (int th = 0; th < TH; ++th) {
      f32x4 u = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int t = 0; t < TD; ++t) {
        const f32x4 w = *reinterpret_cast<const f32x4*>(&W2s[(R * th + n) * S2 + R * t + 4 * part]);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if constexpr (KL) u = TL::mfma(w[r], ap[t][r], u);
          else u = TL::mfma(w[r], a[t][r], u);
        }
        if ((t + 1) % 4 == 0) __builtin_amdgcn_sched_barrier(0);
      }
      hid[th] = (u * hid[th]) * dt;
      store_hidden(p.stash_delta + slot * p.B * hT, th, hid[th]);
      __builtin_amdgcn_sched_barrier(0);
    }

    // ---- elementwise: dW of the forward cell again, the diffusion terms, the reconstruction of y --------------------
    // (the diffusion kind is uniform over the launch: ONE branch around the whole phase, not one per element -- with
    //  the test inside the loops the phase was 70 basic blocks and the register allocator gave up on it)
    // (the backward scheme is a template parameter, not a second uniform branch: with four instances of this phase in
    //  one kernel the 8-wave 128 x 128 variant went from 15 to 210 spilled dwords)
    auto elementwise = [&](auto is_sigmoid) {
      constexpr bool kSigmoid = decltype(is_sigmoid)::value, kMilstein = MILSTEIN;
#pragma unroll
      for (int t = 0; t < TD; ++t) {
        const int ch = R * t + 4 * part;
        float zn[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if constexpr (KL) {
          uint64_t elem = elem0_lane + R * t;
          asm volatile("" : "+v"(elem));
          if (real_d(t)) normal4_straddle<float>(key, elem, cell, 0, kStreamW, zn);
        } else {
          uint64_t quad = quad0 + 4 * t;
          asm volatile("" : "+v"(quad));          // (keeps the step-invariant first Philox round inside the loop)
          if (real_d(t)) normal4_pairs<float>(key, quad, cell, 0, kStreamW, zn);
        }
        const f32x4 cq = lds_quad(cs, ch);
        const f32x4 eq = lds_quad(es, ch);
        const f32x4 bq = lds_quad(b2s, ch);
        [[maybe_unused]] f32x4 hrq, hsq;
        if constexpr (KL) {
          hrq = lds_quad(hrs, ch);
          hsq = lds_quad(hss, ch);
        }
        float rate_terms[4], shift_terms[4];
        [[maybe_unused]] float hrate_terms[4], hshift_terms[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float yt = y[t][r], at = a[t][r], cc = cq[r];
          const float w = zn[r] * sw;
          // g, q = dg/de; then dg/dc = q y, g' = q c; for the sigmoid q' := dq/du = q (1 - 2 s): g'' = q' c^2
          // (affine: q = 1, q' = 0)
          const float u = cc * yt + eq[r];
          float g = u, q = 1.0f, qp = 0.0f;
          if constexpr (kSigmoid) {
            const float sg = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(u * -1.4426950408889634f));
            g = p.diff_amp * sg;
            q = g * (1.0f - sg);
            qp = q * (1.0f - 2.0f * sg);
          }
          const float gp = q * cc;
          const float drift = (f[t][r] + bq[r]) - ito * (g * gp);           // f~
          const float aw = at * w;                                            // a dW
          const float adg = ito * ((at * dt) * g);                           // dt a g   (Ito correction terms)
          const float gpp = qp * (cc * cc);                                  // g''
          float a1 = at + (aw * gp - adg * gpp), y1 = (yt - drift * dt) - g * w;
          // the terms of dL/de, dL/dc: a (dW dg/dtheta - ito dt g dg'/dtheta), with dg/de = q, dg'/de = q' c, dg/dc = q y,
          // dg'/dc = q + q' c y (Milstein: + a v (g' dg/dtheta - g dg'/dtheta))
          const float dgp_de = qp * cc, dgp_dc = dgp_de * yt + q;
          float to_shift = aw * q - adg * dgp_de, to_rate = (aw * q) * yt - adg * dgp_dc;
          if constexpr (kMilstein) {
            const float v = 0.5f * (w * w - ito * dt), av = at * v;
            a1 += av * (gp * gp - g * gpp);
            y1 += v * (g * gp);
            to_shift += av * (gp * q - g * dgp_de);
            to_rate += av * (gp * (q * yt) - g * dgp_dc);
          }
          if constexpr (KL) {
            // the column's share (see MlpAdjKlArgs): u and w as the cotangent phase formed them
            // a_l dt u^2 / safe: none where the divisor is clamped (d safe / d g = 0), none in a padded channel (g may be 0)
            const KlShare kl = kl_share(f[t][r] + bq[r], hrq[r] * yt + hsq[r], g, al, dt, real_d(t));
            const float kq = kl.kq, dtw = kl.dtw;
            a1 = a1 - (hrq[r] * dtw + kq * gp);
            to_shift -= kq * q;
            to_rate -= (kq * q) * yt;
            hrate_terms[r] = row_total(-(dtw * yt) * own_row);
            hshift_terms[r] = row_total(-dtw * own_row);
          }
          rate_terms[r] = row_total(to_rate * own_row);
          shift_terms[r] = row_total(to_shift * own_row);
          a[t][r] = a1;
          y[t][r] = y1;
          // (materialised HERE: left alone, the compiler sinks this arithmetic past the last product of the step and
          //  keeps its inputs alive until then -- 226 spilled dwords in the 8-wave 128 x 128 Milstein variant, 10 with)
          asm volatile("" : "+v"(a[t][r]), "+v"(y[t][r]));
        }
        // summed over the 16 rows of the wave (the 16 lanes of a DPP row hold one channel quad of 16 rows); the row's last
        // lane adds the totals to the wave's LDS accumulators (ds_add_f32: one lane per address, in order per wave)
        if (n == R - 1 && real_d(t)) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            atomicAdd(&wave_sums[ch + r], rate_terms[r]);
            atomicAdd(&wave_sums[D + ch + r], shift_terms[r]);
            if constexpr (KL) {
              atomicAdd(&wave_sums[2 * D + ch + r], hrate_terms[r]);
              atomicAdd(&wave_sums[3 * D + ch + r], hshift_terms[r]);
            }
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    };
    if (sigmoid) elementwise(std::true_type{});
    else elementwise(std::false_type{});

    // ---- a^T += W1 delta^T (rows of W1s, four consecutive hidden units per lane) --------------------------------------
#pragma unroll
    for (int t = 0; t < TD; ++t) {
      f32x4 back = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int th = 0; th < TH; ++th) {
        const f32x4 w = *reinterpret_cast<const f32x4*>(&W1s[(R * t + n) * S1 + R * th + 4 * part]);
#pragma unroll
        for (int r = 0; r < 4; ++r) back = TL::mfma(w[r], hid[th][r], back);
        if ((th + 1) % 4 == 0) __builtin_amdgcn_sched_barrier(0);
      }
      a[t] += back;
      __builtin_amdgcn_sched_barrier(0);
    }
  }

#pragma unroll
  for (int t = 0; t < TD; ++t) {
    store_tile(p.y, t, y[t]);
    store_tile(p.a, t, a[t]);
  }
  // the wave's sums join row `row0` of (row_rate, row_shift)
  for (int i = lane; i < dT; i += 64) {
    p.row_rate[row0 * dT + i] += wave_sums[i];
    p.row_shift[row0 * dT + i] += wave_sums[D + i];
    if constexpr (KL) {
      p.row_hrate[row0 * dT + i] += wave_sums[2 * D + i];
      p.row_hshift[row0 * dT + i] += wave_sums[3 * D + i];
    }
  }
}

// y, a, the f accumulators and act'(z) are 3 x D/4 + H/4 live registers per lane (128 at d = hidden = 128). The large
// shapes exist as 8-wave blocks (two waves per SIMD, 256 registers: at most 10 spilled dwords) and as 4-wave blocks (one
// wave per SIMD, up to 512 registers: no spills); TSDE_ADJ_WAVES=4 picks the latter (default: 8).
//
// The KL instantiation. Five state-sized register arrays are live across the u product (y, a, f, act'(z), a + w): at
// d = hidden = 128 the 8-wave block spills 31-34 dwords (the aligned instantiation: 10), the 4-wave block none -- and the 8-wave
// block is still the faster one (32768 x 128 x 500 forward + backward: 58.0 ms against 61.4 ms,
// profiles/logqp_adjoint_ab.txt), so every shape runs as 8-wave blocks and TSDE_ADJ_WAVES does not reach this instantiation.
template <bool KL>
struct MlpAdjointPolicy {
  using Args = std::conditional_t<KL, MlpAdjKlArgs, MlpAdjArgs>;
  template <int D, int H, int ACT, int NW, bool FULL>
  static hipError_t waves(const Args& p, hipStream_t s) {
    const size_t lds_bytes = MlpLds<16>::bytes(D, H, 3, kAdjExtraFloats<D, NW, KL>);
    return (p.ito & 2) ? launch_rows_per_wave<mlp_adjoint_kernel<D, H, ACT, NW, FULL, true, KL>, NW, 16>(p, lds_bytes, s)
                       : launch_rows_per_wave<mlp_adjoint_kernel<D, H, ACT, NW, FULL, false, KL>, NW, 16>(p, lds_bytes, s);
  }
  template <int D, int H, int ACT, bool FULL>
  static hipError_t launch(const Args& p, hipStream_t s) {
    if constexpr (!KL && (D >= 128 || H >= 256)) {
      static const int waves_env = [] {
        const char* e = getenv("TSDE_ADJ_WAVES");
        return e ? atoi(e) : 0;
      }();
      if (waves_env == 4) return waves<D, H, ACT, 4, FULL>(p, s);
    }
    return waves<D, H, ACT, 8, FULL>(p, s);
  }
};

static void fill_adj_args(MlpAdjArgs& p, void* y, void* a, void* stash_a, void* stash_hid, void* stash_delta, void* stash_y,
                          void* row_rate, void* row_shift, int64_t rows, int64_t d, int64_t h, const void* W1, const void* b1,
                          const void* W2, const void* b2, const void* c, const void* e, int diff_kind, double diff_amp,
                          int ito, const tsde_traj_t* tr, int32_t k_lo, int32_t k_hi, NoiseKey key, const uint64_t* key_dev) {
  fill_mlp_core(p, rows, d, h, W1, b1, W2, c, e, diff_kind, diff_amp, tr, key, key_dev);
  p.y = (float*)y;
  p.a = (float*)a;
  p.stash_a = (float*)stash_a;
  p.stash_hid = (float*)stash_hid;
  p.stash_delta = (float*)stash_delta;
  p.stash_y = (float*)stash_y;
  p.row_rate = (float*)row_rate;
  p.row_shift = (float*)row_shift;
  p.b2 = (const float*)b2;
  p.ito = ito;
  p.k_lo = k_lo;
  p.k_hi = k_hi;
}

hipError_t launch_adjoint_mlp_diag_logqp(void* y, void* a, const void* a_l, void* stash_a, void* stash_hid,
                                         void* stash_delta, void* stash_y, void* row_rate, void* row_shift, void* row_hrate,
                                         void* row_hshift, int64_t rows, int64_t d, int64_t h, const void* W1,
                                         const void* b1, const void* W2, const void* b2, const void* c, const void* e,
                                         const void* hr, const void* hs, int diff_kind, double diff_amp, int act, int ito,
                                         const tsde_traj_t* tr, int32_t k_lo, int32_t k_hi, NoiseKey key,
                                         const uint64_t* key_dev, hipStream_t s) {
  MlpAdjKlArgs p;
  fill_adj_args(p, y, a, stash_a, stash_hid, stash_delta, stash_y, row_rate, row_shift, rows, d, h, W1, b1, W2, b2, c, e,
                diff_kind, diff_amp, ito, tr, k_lo, k_hi, key, key_dev);
  p.a_l = (const float*)a_l;
  p.hr = (const float*)hr;
  p.hs = (const float*)hs;
  p.row_hrate = (float*)row_hrate;
  p.row_hshift = (float*)row_hshift;
  p.bm_stride = d + 1;
  if (rows <= 0 || k_hi <= k_lo) return hipSuccess;
  return mlp_ladder<MlpAdjointPolicy<true>>(p, act, s);
}

hipError_t launch_adjoint_mlp_diag(void* y, void* a, void* stash_a, void* stash_hid, void* stash_delta, void* stash_y,
                                   void* row_rate, void* row_shift, int64_t rows, int64_t d, int64_t h, const void* W1,
                                   const void* b1, const void* W2, const void* b2, const void* c, const void* e,
                                   int diff_kind, double diff_amp, int act, int ito, const tsde_traj_t* tr, int32_t k_lo,
                                   int32_t k_hi, NoiseKey key, const uint64_t* key_dev, hipStream_t s) {
  MlpAdjArgs p;
  fill_adj_args(p, y, a, stash_a, stash_hid, stash_delta, stash_y, row_rate, row_shift, rows, d, h, W1, b1, W2, b2, c, e,
                diff_kind, diff_amp, ito, tr, k_lo, k_hi, key, key_dev);
  if (rows <= 0 || k_hi <= k_lo) return hipSuccess;
  return mlp_ladder<MlpAdjointPolicy<false>>(p, act, s);
}

}  // namespace tsde
