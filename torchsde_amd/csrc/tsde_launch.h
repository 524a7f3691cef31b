// Launchers behind the C ABI (capi.hip hands the dtype on; a launcher dispatches on it once, `by_dtype`).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/torchsde_amd.h"
#include "tsde_bridge.h"
#include "tsde_common.h"
#include "tsde_rng.h"

namespace tsde {

// The dynamic LDS a block can be given, in bytes: the opt-in maximum (what hipFuncSetAttribute can raise a kernel to: 160 KiB
// on gfx950), else the device's default maximum per block, else 64 KiB. Queried once. (The neural launchers' own copies of
// this query went straight to 64 KiB when the opt-in attribute was not answered; they now try the default maximum first.)
inline size_t dynamic_lds_limit() {
  static const size_t limit = [] {
    int dev = 0, bytes = 0;
    if (hipGetDevice(&dev) != hipSuccess) return (size_t)(64 * 1024);
    if (hipDeviceGetAttribute(&bytes, hipDeviceAttributeSharedMemPerBlockOptin, dev) == hipSuccess && bytes > 0)
      return (size_t)bytes;
    if (hipDeviceGetAttribute(&bytes, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) == hipSuccess && bytes > 0)
      return (size_t)bytes;
    return (size_t)(64 * 1024);
  }();
  return limit;
}

// LDS bytes of the kernels that keep a drift AND a diffusion perceptron resident (mlp_general.hip, tsde_neural_rheun.h; the
// staging is tsde_mlp.h's): both first layers, `n_mid` hidden-to-hidden layers, the drift's last layer, the diffusion's last
// layer with its rows padded by `pad`, every bias, and 32 floats of slack behind the output biases (the general-noise
// pipeline requests the biases of the pair after the last one). Rows are padded by 4 floats.
inline size_t two_net_lds_bytes(int D, int H, int outp, int pad, int n_mid) {
  const size_t S1 = H + 4;
  return ((size_t)2 * D * S1 + (size_t)n_mid * H * S1 + (size_t)H * (D + 4) + (size_t)H * (outp + pad) + (size_t)4 * H +
          (size_t)n_mid * H + D + outp + 32) * sizeof(float);
}

// Launch of such a kernel, `Kernel(p, outp)` with 256 threads a block: a block stages the weights once and its four waves walk
// over groups of 16 rows, so the grid is the resident blocks -- the LDS of a CU holds floor(160 KiB / footprint) of them.
// The kernel is allowed the 160 KiB once per instantiation.
template <auto Kernel, typename Args>
hipError_t launch_weights_resident(const Args& p, int outp, size_t lds_bytes, hipStream_t s) {
  if (lds_bytes > dynamic_lds_limit()) return hipErrorInvalidValue;
  constexpr size_t kCuLds = 160 * 1024;
  static bool configured = false;
  if (!configured) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)kCuLds);
    if (e != hipSuccess) return e;
    configured = true;
  }
  const int64_t groups = (p.B + 15) / 16;
  int64_t blocks = (groups + 3) / 4;
  const int64_t per_cu = kCuLds / lds_bytes < 1 ? 1 : (int64_t)(kCuLds / lds_bytes);
  const int64_t resident = 256 * (per_cu > 8 ? 8 : per_cu);
  if (blocks > resident) blocks = resident;
  TSDE_LAUNCH(Kernel, dim3((unsigned)blocks), dim3(256), lds_bytes, s, p, outp);
  return hipGetLastError();
}

// ---- the perceptron-drift kernels (mlp_trajectory.hip, mlp_backward.hip, mlp_adjoint.hip) ----------------------------------

// What the argument structs of all of them hold under the same names -- the weights, b1, the diffusion's c, e, kind and
// amplitude, the schedule's rows and cells, B, d, h and the noise key -- filled from the C-level arguments. (Not a common base
// struct: a base moves these fields to the front of the kernel arguments, and that order is part of what the scalar register
// allocation of the kernels depends on -- profiles/perceptron_frame_resource_usage_notes.txt.)
template <typename Args>
void fill_mlp_core(Args& p, int64_t rows, int64_t d, int64_t h, const void* W1, const void* b1, const void* W2, const void* c,
                   const void* e, int diff_kind, double diff_amp, const tsde_traj_t* tr, NoiseKey key,
                   const uint64_t* key_dev) {
  p.W1 = (const float*)W1;
  p.b1 = (const float*)b1;
  p.W2 = (const float*)W2;
  p.c = (const float*)c;
  p.e = (const float*)e;
  p.diff_kind = diff_kind;
  p.diff_amp = (float)diff_amp;
  p.rows = (const float*)tr->step_rows;
  p.cells = tr->cells;
  p.B = rows;
  p.d = (int32_t)d;
  p.h = (int32_t)h;
  p.key = key;
  p.key_dev = key_dev;
}

// Launch of such a kernel, `Kernel(p)`: a block of NW waves, each owning R batch rows for the whole launch, all sharing one copy
// of the weights in `lds_bytes` of dynamic LDS, which the kernel is allowed once per instantiation.
template <auto Kernel, int NW, int R, typename Args>
hipError_t launch_rows_per_wave(const Args& p, size_t lds_bytes, hipStream_t s) {
  static bool configured = false;
  if (!configured) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)lds_bytes);
    if (e != hipSuccess) return e;
    configured = true;
  }
  const int64_t rows_per_block = NW * R;
  const int64_t blocks = (p.B + rows_per_block - 1) / rows_per_block;
  hipLaunchKernelGGL(Kernel, dim3((unsigned)blocks), dim3(NW * 64), lds_bytes, s, p);
  return hipGetLastError();
}

// The tile sizes of a launch: the smallest D in {32, 64, 128} and H in {32, 64, 128, 256} that hold (p.d, p.h) -- H = 256 for
// D <= 64 only: both weight arrays must fit the LDS of a CU, d * hidden <= 16384 -- the activation, and FULL where nothing is
// padded. Which kernel, how many waves and how much LDS that means is `Policy::launch<D, H, ACT, FULL>(p, s)`.
template <typename Policy, int D, int H, typename Args>
hipError_t mlp_ladder_act(const Args& p, int act, hipStream_t s) {
  const bool full = p.d == D && p.h == H;
  if (act == TSDE_ACT_TANH)
    return full ? Policy::template launch<D, H, TSDE_ACT_TANH, true>(p, s)
                : Policy::template launch<D, H, TSDE_ACT_TANH, false>(p, s);
  if (act == TSDE_ACT_SOFTPLUS)
    return full ? Policy::template launch<D, H, TSDE_ACT_SOFTPLUS, true>(p, s)
                : Policy::template launch<D, H, TSDE_ACT_SOFTPLUS, false>(p, s);
  return hipErrorInvalidValue;
}
template <typename Policy, int D, typename Args>
hipError_t mlp_ladder_h(const Args& p, int act, hipStream_t s) {
  if (p.h <= 32) return mlp_ladder_act<Policy, D, 32>(p, act, s);
  if (p.h <= 64) return mlp_ladder_act<Policy, D, 64>(p, act, s);
  if (p.h <= 128) return mlp_ladder_act<Policy, D, 128>(p, act, s);
  if constexpr (D <= 64) {
    if (p.h <= 256) return mlp_ladder_act<Policy, D, 256>(p, act, s);
  }
  return hipErrorInvalidValue;
}
template <typename Policy, typename Args>
hipError_t mlp_ladder(const Args& p, int act, hipStream_t s) {
  if (p.d <= 32) return mlp_ladder_h<Policy, 32>(p, act, s);
  if (p.d <= 64) return mlp_ladder_h<Policy, 64>(p, act, s);
  if (p.d <= 128) return mlp_ladder_h<Policy, 128>(p, act, s);
  return hipErrorInvalidValue;
}

struct QueryArgs {
  const double* edges;  // device pointer, n_cells + 1 doubles
  int64_t ca, cb;
  double a, b;
  const void* rootW;    // optional pinned (W,H) of the single top-level cell
  const void* rootH;
  const uint64_t* key_dev;  // optional run-time entropy
  const double* ab_dev;     // optional: (a, b) in device memory; then ca, cb, a, b above are ignored
  int64_t n_cells;          // number of cells behind `edges` (needed to locate a, b on the device)
  WalkCfg cfg;
};

// ---- the stepwise launch layer (steps.hip, rheun.hip, adaptive.hip, reduce.hip, milstein_general.hip, brownian.hip) -------

// A launcher takes the state dtype of its C entry point and writes its body once, for a value `t` of that type:
//   return by_dtype(dtype, [&](auto t) { using T = decltype(t); ... });
template <typename Body>
hipError_t by_dtype(int dtype, Body&& body) {
  if (dtype == TSDE_F32) return body(float{});
  if (dtype == TSDE_F64) return body(double{});
  return hipErrorInvalidValue;
}

// The noise of one step as the kernels take it (tsde_common.h: cell_noise): widths rounded to T on the host.
template <typename T>
CellNoise<T> cell_noise_of(const tsde_noise_t* nz) {
  CellNoise<T> c;
  c.dW = (const T*)nz->dW;
  c.dU = (const T*)nz->dU;
  c.key.k0 = (uint32_t)nz->entropy;
  c.key.k1 = (uint32_t)(nz->entropy >> 32);
  c.key.elem0 = nz->elem0;
  c.cell = nz->cell;
  set_width<T>(c, nz->h);
  c.bcast_d = nz->bcast_d;
  c.key_dev = nz->entropy_dev;
  return c;
}

// May a lane take the increments of 4 consecutive elements at once? Generated: they are one Philox quad. External, one row
// for the whole batch: 4 consecutive elements share a row only if d % 4 == 0. External, flat: 16-byte loads of dW (and dU).
inline bool noise_vec_ok(const tsde_noise_t* nz, bool need_u) {
  if (nz->dW == nullptr) return (nz->elem0 % 4) == 0;
  if (nz->bcast_d > 0) return (nz->bcast_d % 4) == 0;
  return aligned16(nz->dW) && (!need_u || aligned16(nz->dU));
}

// The 16-byte path of an elementwise launch: whole groups of 4 and every operand on a 16-byte boundary. A null pointer is an
// absent operand and constrains nothing.
template <typename... Ptr>
bool vec_ok(int64_t n, Ptr... ptrs) {
  return (n % 4 == 0) && (aligned16(ptrs) && ...);
}

constexpr int kSrkIn[5] = {0, 3, 5, 4, 2}, kSrkOut[5] = {0, 3, 3, 2, 1};   // operand counts of SRK (SRID2) stages 1..4

hipError_t launch_normals(int dtype, void* out, int64_t n, NoiseKey key, uint32_t cell, uint64_t node, uint32_t stream_id,
                          hipStream_t s);
hipError_t launch_query(int dtype, void* W, void* U, void* H, int64_t n, NoiseKey key, const QueryArgs& qa, bool have_h,
                        hipStream_t s);
hipError_t launch_cell_increment(int dtype, void* W_out, void* U_out, int64_t n, const tsde_noise_t* nz, hipStream_t s);
hipError_t launch_step_diag(int dtype, void* y1, const void* y0, const void* f, const void* g, int64_t n, double cf, double cg,
                            const tsde_noise_t* nz, hipStream_t s);
hipError_t launch_step_prod(int dtype, void* y1, const void* y0, const void* f, const void* gp, int64_t n, double cf, double cg,
                            hipStream_t s);
hipError_t launch_step_general(int dtype, void* y1, const void* y0, const void* f, const void* g, int64_t B, int64_t d,
                               int64_t m, double ca, double cf, double cg, int weight_mode, double cw, double cu, double rdt,
                               const tsde_noise_t* nz, hipStream_t s);
hipError_t launch_step_shared(int dtype, void* y1, const void* y0, const void* f, const void* S, int64_t B, int64_t d,
                              int64_t m, double ca, double cf, double cg, int weight_mode, double cw, double cu, double rdt,
                              const tsde_noise_t* nz, hipStream_t s);
hipError_t launch_milstein_v(int dtype, void* v_out, void* W_out, const void* g, int64_t n, double dt, int ito, double scale,
                             const tsde_noise_t* nz, hipStream_t s);
hipError_t launch_milstein_diag(int dtype, void* y1, const void* y0, const void* f, const void* g, const void* gdg, int64_t n,
                                double dt, const tsde_noise_t* nz, hipStream_t s);
hipError_t launch_milstein_gf_prime(int dtype, void* yp, const void* y0, const void* f, const void* g, int64_t n, double dt,
                                    double sqrt_dt, int ito, hipStream_t s);
hipError_t launch_milstein_gf_diag(int dtype, void* y1, const void* y0, const void* f, const void* g, const void* gp, int64_t n,
                                   double dt, double sqrt_dt, int ito, const tsde_noise_t* nz, hipStream_t s);
hipError_t launch_srk_stage(int dtype, int stage, void* const out[3], const void* const in[5], int64_t n, double dt, double rdt,
                            double sqrt_dt, const tsde_noise_t* nz, hipStream_t s);
hipError_t launch_milstein_gf_general_support(int dtype, void* yk, const void* y0, const void* f, const void* g, int64_t B,
                                              int64_t d, int64_t m, double dt, double sqrt_dt, int ito, hipStream_t s);
hipError_t launch_milstein_gf_general_correction(int dtype, void* corr, const void* g, const void* gk, const void* I, int64_t B,
                                                 int64_t d, int64_t m, double sqrt_dt, hipStream_t s);
hipError_t launch_aug_segments(int dtype, const tsde_seg_t* segs, int nseg, double cF, double cG, hipStream_t s, int* taken);
hipError_t launch_interp(int dtype, void* out, const void* ya, const void* yb, int64_t n, double w0, double w1, hipStream_t s);
// rheun.hip
hipError_t launch_heun_final(int dtype, void* y1, const void* y0, const void* f, const void* fp, const void* g, const void* gp,
                             int64_t n, double dt, int mode, int prod, const tsde_noise_t* nz, hipStream_t s);
hipError_t launch_iterated_integrals(int dtype, void* I, const void* W, const void* A, int64_t B, int64_t m, double dt, int ito,
                                     hipStream_t s);
hipError_t launch_levy_area(int dtype, void* A, const void* W, const void* H, int64_t B, int64_t m, double h, int foster,
                            NoiseKey key, const uint64_t* key_dev, uint32_t cell, uint64_t node, hipStream_t s, int fuse = 0,
                            double dt = 0.0, int ito = 0);
hipError_t launch_rheun_z(int dtype, void* z1, const void* y0, const void* z0, const void* f0, const void* g0, int64_t n,
                          double dt, double sgn, const tsde_noise_t* nz, hipStream_t s);
hipError_t launch_rheun_y(int dtype, void* y1, const void* y0, const void* f0, const void* f1, const void* g0, const void* g1,
                          int64_t n, double half_dt, double sgn, const tsde_noise_t* nz, hipStream_t s);
hipError_t launch_lincomb2(int dtype, void* out, const void* x, const void* y, int64_t n, double a, double b, hipStream_t s);
hipError_t launch_rheun_adj_a(int dtype, void* af0_out, void* ag0_out, const void* ay, const void* af0, const void* ag0,
                              int64_t n, double half_dt, const tsde_noise_t* nz, hipStream_t s);
hipError_t launch_rheun_adj_b(int dtype, void* ay1, void* az1, void* af1, void* ag1, const void* ay, const void* az0,
                              const void* vjp_z, int64_t n, double dt, double half_dt, const tsde_noise_t* nz, hipStream_t s);
// reduce.hip
hipError_t launch_error_norm(int dtype, double* out, double* workspace, const void* yf, const void* yh, int64_t n, double rtol,
                             double atol, double eps, hipStream_t s);
// adaptive.hip
hipError_t launch_adaptive_begin(int dtype, double* ctl, void* scal, double out_t, const double* out_times, int n_out,
                                 const double* fracs, int n_fracs, hipStream_t s);
hipError_t launch_adaptive_control(int dtype, double* ctl, void* scal, const double* error, const double* out_times,
                                   double* accept_log, int log_capacity, const double* fracs, int n_fracs, hipStream_t s);
hipError_t launch_adaptive_emit(int dtype, const void* ys_slot, const void* prev_y, const void* curr_y, int64_t n,
                                const double* ctl, const double* out_times, hipStream_t s);
hipError_t launch_adaptive_commit(int dtype, void* prev_y, void* curr_y, const void* y_next, int64_t n, const void* scal,
                                  hipStream_t s);
hipError_t launch_merge_halves(int dtype, void* W, void* U, const void* Wa, const void* Ha, const void* Wb, const void* Hb,
                               int64_t n, const double* ctl, double ha, double hb, hipStream_t s);
// trajectory.hip
hipError_t launch_trajectory_affine_diag(int dtype, void* ys, void* sens, const void* y0, int64_t rows, int64_t d,
                                         const void* a, const void* b, const void* c, const void* e, int64_t cstride,
                                         int method, const tsde_traj_t* tr, NoiseKey key, const uint64_t* key_dev,
                                         hipStream_t s);
hipError_t launch_trajectory_expr_diag(int dtype, void* ys, const void* y0, int64_t rows, int64_t d, const void* const coef[8],
                                       int64_t cstride, int f_kind, int g_kind, int method, const tsde_traj_t* tr, NoiseKey key,
                                       const uint64_t* key_dev, hipStream_t s);
hipError_t launch_trajectory_prog_diag(int dtype, void* ys, void* sens, const int8_t* param_slot, const void* y0, int64_t rows,
                                       int64_t d, const uint32_t* code, int f_len, int g_len, int dg_len, const void* consts,
                                       int n_const, int scalar_noise, int method, const tsde_traj_t* tr, NoiseKey key,
                                       const uint64_t* key_dev, hipStream_t s);
hipError_t launch_trajectory_prog_additive(int dtype, void* ys, const void* y0, int64_t rows, int64_t d, int64_t m,
                                           const uint32_t* code, int f_len, const void* consts, int n_const, const void* gtab,
                                           int time_dependent, int method, const tsde_traj_t* tr, NoiseKey key,
                                           const uint64_t* key_dev, hipStream_t s);
// mlp_trajectory.hip
hipError_t launch_trajectory_mlp_diag(void* ys, const void* y0, int64_t rows, int64_t d, int64_t h, const void* W1,
                                      const void* b1, const void* W2, const void* b2, const void* c, const void* e,
                                      int diff_kind, double diff_amp, int act, int method, const tsde_traj_t* tr,
                                      NoiseKey key, const uint64_t* key_dev, hipStream_t s);
hipError_t launch_trajectory_mlp_diag_logqp(void* ys, void* logqp, const void* y0, int64_t rows, int64_t d, int64_t h,
                                            const void* W1, const void* b1, const void* W2, const void* b2, const void* c,
                                            const void* e, const void* hr, const void* hs, int diff_kind, double diff_amp,
                                            int act, int method, const tsde_traj_t* tr, NoiseKey key,
                                            const uint64_t* key_dev, hipStream_t s);
// mlp_general.hip
hipError_t launch_trajectory_mlp_general(void* ys, const void* y0, int64_t rows, int64_t d, int64_t m, int noise,
                                         const tsde_mlp_t* drift, const tsde_mlp_t* diffusion, int method,
                                         const tsde_traj_t* tr, NoiseKey key, const uint64_t* key_dev, hipStream_t s);
hipError_t launch_trajectory_mlp_additive(void* ys, const void* y0, int64_t rows, int64_t d, int64_t m, const tsde_mlp_t* drift,
                                          const void* gtab, int time_dependent, int method, const tsde_traj_t* tr,
                                          NoiseKey key, const uint64_t* key_dev, hipStream_t s);
size_t neural_footprint(int64_t d, int64_t m, int64_t hf, int64_t hg, int64_t out, int noise);
// mlp_backward.hip
hipError_t launch_trajectory_mlp_diag_backward(void* lam, void* stash_lam, void* stash_hid, void* stash_delta,
                                               void* row_rate, void* row_shift, const void* ys_all,
                                               int32_t ys_first, const void* grad_ys, const int32_t* grad_step,
                                               const void* grad_w, int32_t grad_last,
                                               int64_t rows, int64_t d, int64_t h, const void* W1, const void* b1,
                                               const void* W2, const void* c, const void* e, int diff_kind,
                                               double diff_amp, int act, int method, const tsde_traj_t* tr,
                                               int32_t k_lo, int32_t k_hi, NoiseKey key, const uint64_t* key_dev,
                                               hipStream_t s);
hipError_t launch_trajectory_mlp_diag_logqp_backward(void* lam, void* a_l, void* stash_lam, void* stash_hid,
                                                     void* stash_delta, void* row_rate, void* row_shift, void* row_hrate,
                                                     void* row_hshift, const void* ys_all, int32_t ys_first,
                                                     const void* grad_ys, const void* grad_logqp, const int32_t* grad_step,
                                                     const void* grad_w, int32_t grad_last, int64_t rows, int64_t d, int64_t h,
                                                     const void* W1,
                                                     const void* b1, const void* W2, const void* b2, const void* c,
                                                     const void* e, const void* hr, const void* hs, int diff_kind,
                                                     double diff_amp, int act, int method, const tsde_traj_t* tr,
                                                     int32_t k_lo, int32_t k_hi, int64_t bm_stride, NoiseKey key,
                                                     const uint64_t* key_dev, hipStream_t s);
// mlp_adjoint.hip
hipError_t launch_adjoint_mlp_diag(void* y, void* a, void* stash_a, void* stash_hid, void* stash_delta, void* stash_y,
                                   void* row_rate, void* row_shift, int64_t rows, int64_t d, int64_t h, const void* W1,
                                   const void* b1, const void* W2, const void* b2, const void* c, const void* e,
                                   int diff_kind, double diff_amp, int act, int ito, const tsde_traj_t* tr, int32_t k_lo,
                                   int32_t k_hi, NoiseKey key, const uint64_t* key_dev, hipStream_t s);
hipError_t launch_adjoint_mlp_diag_logqp(void* y, void* a, const void* a_l, void* stash_a, void* stash_hid,
                                         void* stash_delta, void* stash_y, void* row_rate, void* row_shift, void* row_hrate,
                                         void* row_hshift, int64_t rows, int64_t d, int64_t h, const void* W1,
                                         const void* b1, const void* W2, const void* b2, const void* c, const void* e,
                                         const void* hr, const void* hs, int diff_kind, double diff_amp, int act, int ito,
                                         const tsde_traj_t* tr, int32_t k_lo, int32_t k_hi, NoiseKey key,
                                         const uint64_t* key_dev, hipStream_t s);
hipError_t launch_gram_partials(void* partials, void* colsums, const void* A, int64_t lda, const void* Bm, int64_t ldb,
                                int64_t K, int64_t M, int64_t N, int32_t blocks, hipStream_t s);
// graph_nodes.hip: memset nodes of a captured, not yet instantiated graph -> fill-kernel nodes with the same edges
hipError_t memset_nodes_to_kernels(hipGraph_t graph, int* n_memset, int* n_replaced);
// neural_rheun.hip
hipError_t launch_rheun_mlp_forward(void* ys, void* z_out, const void* y0, int64_t rows, int64_t d, int64_t m, int noise,
                                    const tsde_deep_mlp_t* drift, const tsde_deep_mlp_t* diffusion, int method,
                                    const tsde_traj_t* tr, const void* times, NoiseKey key, const uint64_t* key_dev,
                                    hipStream_t s);
hipError_t launch_rheun_mlp_backward(const tsde_rheun_state_t* state, const tsde_rheun_stash_t* stash, const void* ys_all,
                                     const void* grad_ys, int64_t rows, int64_t d, int64_t m, int noise,
                                     const tsde_deep_mlp_t* drift, const tsde_deep_mlp_t* diffusion, const tsde_traj_t* tr,
                                     const void* times, int j_hi, int j_lo, NoiseKey key, const uint64_t* key_dev,
                                     hipStream_t s);
hipError_t launch_rheun_last_layer_grad(void* gw, void* gb, const void* hid, const void* p, const void* q, const void* wa,
                                        const void* wb, int64_t N, int64_t d, int64_t m, const tsde_deep_mlp_t* net,
                                        int32_t stride_h, int32_t stride_d, int32_t stride_m, int32_t row_blocks, hipStream_t s);
size_t rheun_footprint(int64_t d, int64_t m, int64_t hf, int64_t hg, int64_t out, int noise, int nmf, int nmg);
}  // namespace tsde
