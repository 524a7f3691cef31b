// Shared pieces of the perceptron kernels:
//   perceptron drift (mlp_trajectory.hip: sampling; mlp_backward.hip, mlp_adjoint.hip: its gradients): the two f32 MFMA tile
//     shapes, the activations on the hardware transcendentals, and the LDS footprint;
//   drift AND diffusion perceptrons (mlp_general.hip, tsde_neural_rheun.h): everything the two kernels do BEFORE their step
//     loops -- the staging of both nets into LDS, the padded (and pair-interleaved) layout of the diffusion's last layer --
//     and the two helpers their step bodies share, the operand-read schedule and the out-of-line single draw. The step
//     bodies themselves are hand-scheduled per kernel and are not shared.
#pragma once
#include "tsde_common.h"

namespace tsde {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// Activations on the hardware transcendentals (v_exp_f32 / v_log_f32 / v_rcp_f32, ~1 ulp each): the libm forms
// (tanhf, log1pf(expf)) expand to ~100 instructions with divergent special-case branches, which made the
// activation -- not the matrix products -- the longest part of a step. Error against float64, ABSOLUTE where the result is
// below 1 and RELATIVE above (relative error near 0 is unbounded for any form that goes through exp), worst over all binades
// 2^-30 .. 2^7 and the saturation / threshold / overflow points -- with correctly rounded primitives, then as measured on
// gfx950 (profiles/neural_activation_accuracy.txt; tests/test_gpu_neural_activations.py holds every site to twice the first
// figure plus 2^-24):
//   tanh value      1.7e-7  1.8e-7        tanh slope 1 - v^2          3.4e-7  3.2e-7
//   softplus value  1.5e-7  1.9e-7        softplus slope              7.9e-8  8.4e-8   (1 - rcp(1 + ex); ex * rcp(1 + ex): 7.6e-8)
//   sigmoid value   7.9e-8  8.3e-8        sigmoid slope s (1 - s)     7.4e-8  7.4e-8
//   LipSwish value  1.2e-7  1.2e-7        LipSwish slope              8.6e-7  8.6e-7   (x (1 - s) near x = 16.6; torch's: the same)
// (softplus and LipSwish values are that close to the VALUE: absolutely they are off by up to 1.6e-6 / 1.2e-6 near x = 11 .. 16,
// where an ulp of the value is 1e-6.) No form returns a NaN or an infinity for a finite argument. All of it is well inside the
// tolerance at which these kernels are compared with the stepwise path (summation order already differs).
template <int ACT>
TSDE_D float activate(float x) {
  constexpr float kLog2e = 1.4426950408889634f, kLn2 = 0.6931471805599453f;
  if constexpr (ACT == TSDE_ACT_TANH) {
    // tanh(x) = 1 - 2 / (exp(2x) + 1); exp(2x) = 2^(2x log2 e); saturates cleanly to +-1
    const float e2x = __builtin_amdgcn_exp2f(x * (2.0f * kLog2e));
    return 1.0f - 2.0f * __builtin_amdgcn_rcpf(e2x + 1.0f);
  } else {
    // softplus, torch's threshold-20 form (aten/src/ATen/native/cuda/ActivationSoftplusKernel.cu): log(1 + e^x)
    const float ex = __builtin_amdgcn_exp2f(x * kLog2e);
    const float sp = __builtin_amdgcn_logf(1.0f + ex) * kLn2;
    return x > 20.0f ? x : sp;
  }
}

// The activation together with its derivative, from the same exponential (mlp_backward.hip).
template <int ACT>
TSDE_D void activate_with_slope(float x, float& value, float& slope) {
  constexpr float kLog2e = 1.4426950408889634f, kLn2 = 0.6931471805599453f;
  if constexpr (ACT == TSDE_ACT_TANH) {
    const float e2x = __builtin_amdgcn_exp2f(x * (2.0f * kLog2e));
    value = 1.0f - 2.0f * __builtin_amdgcn_rcpf(e2x + 1.0f);
    slope = 1.0f - value * value;
  } else {
    // d/dx log(1 + e^x) = e^x / (1 + e^x) = 1 - 1 / (1 + e^x); torch's backward returns exactly 1 past the threshold
    const float ex = __builtin_amdgcn_exp2f(x * kLog2e);
    const float sp = __builtin_amdgcn_logf(1.0f + ex) * kLn2;
    value = x > 20.0f ? x : sp;
    slope = x > 20.0f ? 1.0f : 1.0f - __builtin_amdgcn_rcpf(1.0f + ex);
  }
}

typedef float f32x4 __attribute__((ext_vector_type(4)));

// The two f32 MFMA shapes. R = rows of the batch one wave owns = the tile edge.
//   R = 32: v_mfma_f32_32x32x2_f32, 16 accumulator registers per tile, two lane halves  (K = 2 per instruction)
//   R = 16: v_mfma_f32_16x16x4_f32,  4 accumulator registers per tile, four lane quarters (K = 4 per instruction)
// `part` = lane / R selects the K index a lane feeds and the rows of the accumulator it holds; for a fixed register
// the parts hold channels that differ by 4, which is the K grouping both operands are addressed with.
template <int R>
struct Tile;
template <>
struct Tile<32> {
  static constexpr int kRegs = 16, kQuads = 4;
  using acc_t = f32x16;
  TSDE_D static constexpr int row(int r, int part) { return (r & 3) + 8 * (r >> 2) + 4 * part; }
  TSDE_D static constexpr int quad_base(int q, int part) { return 8 * q + 4 * part; }   // channels of regs 4q..4q+3
  TSDE_D static acc_t mfma(float a, float b, acc_t c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
};
template <>
struct Tile<16> {
  static constexpr int kRegs = 4, kQuads = 1;
  using acc_t = f32x4;
  TSDE_D static constexpr int row(int r, int part) { return 4 * part + r; }
  TSDE_D static constexpr int quad_base(int q, int part) { return 4 * part; }
  TSDE_D static acc_t mfma(float a, float b, acc_t c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
};

// Four consecutive per-channel constants (biases, diffusion coefficients) from LDS, re-read at every use: the index is
// made opaque so that the loads are NOT hoisted out of the step loop -- hoisted, the constants of all tiles pin more
// than a hundred registers per lane for the whole solve (one ds_read_b128 per quad and step is noise next to the
// hundreds of operand reads of the matrix products).
TSDE_D f32x4 lds_quad(const float* base, int index) {
  asm volatile("" : "+v"(index));
  return *reinterpret_cast<const f32x4*>(base + index);
}

// Diagonal diffusion of one channel and its derivative w.r.t. the shift e (q: then dg/dc = q*y and dg/dy = q*c):
//   affine   g = c*y + e                      q = 1
//   sigmoid  g = amp * sigmoid(c*y + e)       q = amp * s * (1 - s)
// `sigmoid` is uniform over the launch (a scalar branch); the explicitly scheduled sampling kernel passes a constant.
struct DiffusionValue {
  float g, q;
};
TSDE_D DiffusionValue diffusion_value(bool sigmoid, float amp, float c, float e, float y) {
  const float u = c * y + e;
  DiffusionValue v = {u, 1.0f};
  if (sigmoid) {
    const float s = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(u * -1.4426950408889634f));
    v.g = amp * s;
    v.q = v.g * (1.0f - s);
  }
  return v;
}

// The divisor of misc.stable_division (misc.py:66-68), which the KL column of a logqp solve divides f - h by: g itself, or
// 1e-7 with g's sign where |g| <= 1e-7 (the reference's `sign`: 0 at 0).
TSDE_D float stable_divisor(float g) {
  const float sign = g > 0.0f ? 1.0f : (g < 0.0f ? -1.0f : 0.0f);
  return fabsf(g) > 1e-7f ? g : 1e-7f * sign;
}

// Sum of `v` over the 16 lanes of a DPP row, valid in the row's last lane (inclusive scan by row_shr 1, 2, 4, 8; lanes
// shifted in from outside the row read 0).
TSDE_D float row_total(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x111, 0xf, 0xf, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x112, 0xf, 0xf, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x114, 0xf, 0xf, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x118, 0xf, 0xf, true));
  return v;
}

// What the KL column l (l' = 0.5 sum_i u_i^2, u = (f - h) / safe(g)) hands back to one channel of a reverse step, given the
// column's cotangent a_l -- the stochastic adjoint (mlp_adjoint.hip) and back-propagation through the solver
// (mlp_backward.hip) use the same three numbers:
//   w   = a_l u / safe                 the drift network sees its cotangent + w; the prior's h = hr y + hs sees -w
//   dtw = dt w                         dL/dy += -hr dtw;  dL/dhr += -dtw y;  dL/dhs += -dtw
//   kq  = a_l dt u^2 / safe            dL/dy += -kq g';   dL/dtheta_g += -kq dg/dtheta
// The replaced divisor is a constant (no kq where |g| <= 1e-7); a padded channel (`real` false: g may be 0 there) has no share
// in dtw and kq, and its w is the caller's to drop.
struct KlShare {
  float w, dtw, kq;
};
TSDE_D float kl_cotangent(float f, float h, float g, float al) {
  const float safe = stable_divisor(g);
  const float uk = (f - h) / safe;
  return (al * uk) / safe;
}
TSDE_D KlShare kl_share(float f, float h, float g, float al, float dt, bool real) {
  const float safe = stable_divisor(g);
  const float uk = (f - h) / safe;
  const float wk = (al * uk) / safe;
  KlShare s;
  s.w = wk;
  s.kq = (real && fabsf(g) > 1e-7f) ? ((al * dt) * (uk * uk)) / safe : 0.0f;
  s.dtw = real ? dt * wk : 0.0f;
  return s;
}

// ---- drift and diffusion perceptrons: mlp_general.hip, tsde_neural_rheun.h ------------------------------------------------

// One normal of the field, out of line: the element-by-element paths (d % 4 != 0, m not a tile width, an unaligned field) are
// rare and must not cost the common path registers.
inline __device__ __noinline__ float draw_one(NoiseKey key, uint64_t elem, uint32_t cell, uint32_t stream) {
  return normal1<float>(key, elem, cell, 0, stream);
}

// Schedule of a straight-line region of READS LDS operand reads, each feeding PER matrix instructions: the first few reads
// go out ahead, then every group of PER MFMAs is followed by one more read -- left alone, hipcc emits read -> wait -> PER
// MFMAs and the wave (there is ONE per SIMD at the configs[2] shape, nothing else to switch to) sits out the LDS latency
// once per read: 18.7 ms per 1000-step solve at 16384 x 32 x 16 before, see DESIGN.md for after.
template <int READS, int PER>
TSDE_D void reads_ahead() {
  constexpr int AHEAD = READS < 4 ? READS : 4;
  __builtin_amdgcn_sched_group_barrier(0x100, AHEAD, 0);
#pragma unroll
  for (int i = 0; i < READS; ++i) {
    __builtin_amdgcn_sched_group_barrier(0x008, PER, 0);
    if (i < READS - AHEAD) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
  }
  __builtin_amdgcn_sched_barrier(0);
}

// Staging of both nets into LDS (called by all 256 threads of a block, before its barrier), zero-padded to the tile sizes D and
// H: padded hidden units see zero weights both ways, padded state channels are never read back. Rows are padded by 4 floats
// (the four lane quarters of a wave read rows 4 apart: conflict-free ds_read_b32). `Net`: NeuralNet or DeepNet -- the same field
// names; `dT`: the real state width. Two calls, weights and biases: the kernels stage the diffusion's last layer in between,
// and the order of these loops is part of what the register allocation of the step bodies depends on -- keep it (DESIGN.md
// section 4).
//   stage_two_nets: both first layers [input channel][hidden unit] and the drift's last layer [hidden unit][state channel]
template <int D, int H, typename Net>
TSDE_D void stage_two_nets(const Net& f, const Net& g, int dT, float* W1f, float* W1g, float* W2f) {
  constexpr int S1 = H + 4, S2F = D + 4;
  const int hf = f.hidden, hg = g.hidden;
  for (int i = threadIdx.x; i < D * H; i += 256) {
    const int k = i / H, u = i % H;
    W1f[k * S1 + u] = (k < dT && u < hf) ? f.w1[k * hf + u] : 0.0f;
    W1g[k * S1 + u] = (k < dT && u < hg) ? g.w1[k * hg + u] : 0.0f;
    const int u2 = i / D, c = i % D;
    W2f[u2 * S2F + c] = (u2 < hf && c < dT) ? f.w2[u2 * dT + c] : 0.0f;
  }
}
//   stage_two_nets_biases: first-layer biases and time columns (b1, w1t) of both nets, and the drift's output bias
template <int D, int H, typename Net>
TSDE_D void stage_two_nets_biases(const Net& f, const Net& g, int dT, float* b1f, float* wtf, float* b1g, float* wtg,
                                  float* b2f) {
  const int hf = f.hidden, hg = g.hidden;
  for (int i = threadIdx.x; i < H; i += 256) {
    b1f[i] = i < hf ? f.b1[i] : 0.0f;
    wtf[i] = (i < hf && f.w1t) ? f.w1t[i] : 0.0f;
    b1g[i] = i < hg ? g.b1[i] : 0.0f;
    wtg[i] = (i < hg && g.w1t) ? g.w1t[i] : 0.0f;
  }
  for (int i = threadIdx.x; i < D; i += 256) b2f[i] = i < dT ? f.b2[i] : 0.0f;
}

// Where output o of the diffusion's padded last layer comes from in the net's own last layer (weights and biases alike).
// General noise: the net's outputs are (i, j) row-major with m REAL Brownian channels; the tiles want i * M + j with M the
// channel count padded to a tile width (padded channels: zero weights, zero bias, zero increments). Any other noise: output o
// itself, up to the net's width outT.
struct OutputSource {
  bool have;
  int src;
};
template <bool GENERAL>
TSDE_D OutputSource padded_output(int o, int M, int dT, int m, int outT) {
  if constexpr (GENERAL) {
    const int ci = o / M, cj = o % M;
    return {ci < dT && cj < m, ci * m + cj};
  }
  return {o < outT, o};
}

// General noise, exact f32: the diffusion net's second layer sits in LDS with the two tiles of a PAIR interleaved -- element
// (unit u, output o = 16 tile + c) at u * stride + 32 (tile / 2) + 2 c + (tile & 1), which is pair_slot(o) -- so that a lane's
// two A operands of a unit are ONE ds_read_b64, and with a row stride of 8 (mod 16) floats: a b64 read is served in two halves
// of 32 lanes, the two lane quarters of a half read units 4 apart, 4 * stride = 32 (mod 64) banks puts them on the two halves of
// the banks. For D <= 32 the stride is D * M + 8 whatever the real width: every row offset of the products is then an immediate
// of the read (the address arithmetic between the matrix instructions cost more than the reads:
// profiles/r6_microbench_mfma_fillers.txt).
template <int D, int MODE, bool SPLIT>
struct PairLayout {
  static constexpr bool kOn = MODE >= 4 && !SPLIT;
  static constexpr bool kFixed = kOn && D <= 32;
  static constexpr int kPad = kOn ? 8 : 4;
};
TSDE_D int pair_slot(int o) { return 32 * (o >> 5) + 2 * (o & 15) + ((o >> 4) & 1); }

// ---- perceptron drift: mlp_trajectory.hip, mlp_backward.hip, mlp_adjoint.hip ------------------------------------------------

// The LDS of a block, in floats from its start: W1s (D rows of H + kPad), W2s (H rows of D + kPad), b1s (H), then `vectors`
// per-channel arrays of D (b2 / c / e, ...), then `extra` floats of the kernel's own (the adjoint's per-wave sums). The kernels
// carve their pointers with w2 / b1 / vec and the launchers ask `bytes` for the same (vectors, extra): one formula.
template <int R>
struct MlpLds {
  static constexpr int kPad = (R == 16) ? 4 : 0;
  static constexpr int w2(int d, int h) { return d * (h + kPad); }
  static constexpr int b1(int d, int h) { return w2(d, h) + h * (d + kPad); }
  static constexpr int vec(int d, int h, int i) { return b1(d, h) + h + i * d; }
  static constexpr size_t bytes(int d, int h, int vectors = 3, int extra = 0) {
    return (size_t)(vec(d, h, vectors) + extra) * sizeof(float);
  }
};

// Staging of the net into LDS by the two gradient kernels (called by all THREADS threads of a block, before its barrier):
// W1s[channel][hidden unit], W2s[hidden unit][channel] and b1s, zero-padded from (dT, hT) to the tile sizes (D, H) -- padded
// hidden units see zero weights both ways, padded state channels are never read back. As stage_two_nets: the order of these
// loops is part of what the register allocation of the step bodies depends on. The per-channel vectors stay with each kernel,
// and so does the whole staging of the sampling kernel, whose explicitly scheduled form stores the transposes.
template <int D, int H, int R, int THREADS>
TSDE_D void stage_perceptron(float* lds, const float* W1, const float* W2, const float* b1, int dT, int hT) {
  using L = MlpLds<R>;
  constexpr int S1 = H + L::kPad, S2 = D + L::kPad;
  float *W1s = lds, *W2s = lds + L::w2(D, H), *b1s = lds + L::b1(D, H);
  for (int i = threadIdx.x; i < D * H; i += THREADS) {
    const int k1 = i / H, m1 = i % H, k2 = i / D, m2 = i % D;
    W1s[k1 * S1 + m1] = (k1 < dT && m1 < hT) ? W1[k1 * hT + m1] : 0.0f;
    W2s[k2 * S2 + m2] = (k2 < hT && m2 < dT) ? W2[k2 * dT + m2] : 0.0f;
  }
  for (int i = threadIdx.x; i < H; i += THREADS) b1s[i] = i < hT ? b1[i] : 0.0f;
}

}  // namespace tsde
