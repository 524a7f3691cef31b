// Whole-trajectory kernel for closed-form diagonal SDEs on gfx950.
//
// When drift and diffusion are known in closed form (affine here: f = a*y + b, g = c*y + e, per state channel),
// nothing in the reference's stepping loop (torchsde/_core/base_solver.py:114-134) has to leave the chip between
// steps: every (batch row, channel) element is an independent scalar recursion. One lane owns 4 consecutive
// elements, keeps them in registers for ALL steps of the solve, draws each step's Brownian increment from the
// counter RNG (the same (entropy, element, cell) field the per-step kernels use) and only touches HBM to read
// y0 and to write the requested output times. HBM traffic drops from 4 streams per step to ~0, and the bound
// becomes the Philox/Box-Muller ALU work.
//
// The arithmetic is the per-step kernels' arithmetic (tsde_schemes.h), so the results are bit-identical to the
// stepwise path with the same SDE evaluated by torch ops:
//   Euler      _core/methods/euler.py:31-36         Midpoint  _core/methods/midpoint.py:31-43
//   Milstein   _core/methods/milstein.py:52-74      SRK       _core/methods/srk.py:57-88 (SRID2)
//   outputs    _core/base_solver.py:131-134 + _core/interp.py:19-26 (linear interpolation inside a step)
//
// Gradients: the same kernel instantiated on forward-mode dual numbers carries, next to every state element, its
// path-wise sensitivities d y / d (y0, a, b, c, e) through exactly the same operations (the recursions are
// element-wise, so each tangent is one more scalar recursion in registers). This is what back-propagation
// through the solver (ordinary autograd through torchsde.sdeint) computes for such an SDE, in the same single launch.
#include <type_traits>

#include "tsde_common.h"
#include "tsde_launch.h"
#include "tsde_schemes.h"

namespace tsde {

constexpr int kSens = 5;   // tangents per element: d/dy0, d/da, d/db, d/dc, d/de

// Value + tangents. Only the operations an affine SDE needs: the state is never multiplied by the state.
template <typename T>
struct Dual {
  T v;
  T d[kSens];
  Dual() = default;
  TSDE_D explicit Dual(T value) : v(value) {
#pragma unroll
    for (int i = 0; i < kSens; ++i) d[i] = (T)0;
  }
};

// A coefficient: a plain value whose own tangent slot K is 1 (and every other 0), kept symbolic so that products and
// sums with it cost one extra add instead of a dense tangent update.
template <typename T, int K>
struct Seed {
  T v;
};

template <typename T>
TSDE_D Dual<T> operator+(const Dual<T>& x, const Dual<T>& y) {
  Dual<T> r;
  r.v = x.v + y.v;
#pragma unroll
  for (int i = 0; i < kSens; ++i) r.d[i] = x.d[i] + y.d[i];
  return r;
}
template <typename T>
TSDE_D Dual<T> operator+(const Dual<T>& x, T s) {
  Dual<T> r = x;
  r.v = x.v + s;
  return r;
}
template <typename T>
TSDE_D Dual<T> operator*(const Dual<T>& x, T s) {
  Dual<T> r;
  r.v = x.v * s;
#pragma unroll
  for (int i = 0; i < kSens; ++i) r.d[i] = x.d[i] * s;
  return r;
}
template <typename T>
TSDE_D Dual<T> operator*(T s, const Dual<T>& x) {
  Dual<T> r;
  r.v = s * x.v;
#pragma unroll
  for (int i = 0; i < kSens; ++i) r.d[i] = s * x.d[i];
  return r;
}
template <typename T, int K>
TSDE_D Dual<T> operator*(const Seed<T, K>& p, const Dual<T>& x) {
  Dual<T> r;
  r.v = p.v * x.v;
#pragma unroll
  for (int i = 0; i < kSens; ++i) r.d[i] = p.v * x.d[i];
  r.d[K] = r.d[K] + x.v;
  return r;
}
template <typename T, int K>
TSDE_D Dual<T> operator*(const Dual<T>& x, const Seed<T, K>& p) {
  Dual<T> r;
  r.v = x.v * p.v;
#pragma unroll
  for (int i = 0; i < kSens; ++i) r.d[i] = x.d[i] * p.v;
  r.d[K] = r.d[K] + x.v;
  return r;
}
template <typename T, int K>
TSDE_D Dual<T> operator+(const Dual<T>& x, const Seed<T, K>& p) {
  Dual<T> r = x;
  r.v = x.v + p.v;
  r.d[K] = r.d[K] + (T)1;
  return r;
}

// ---- what the five kernels of this file share --------------------------------------------------------------------------
// Every kernel below is the same loop: a lane loads its elements of y0, and per step reads the step's scalars (`step_row`),
// draws its Brownian increments (`draw_increment`), advances its state with its own model, and at the few steps that meet
// an output time writes the outputs (`emit_outputs`). The host side is shared likewise: `traj_common` fills the common
// arguments, `may_vec` decides on the 4-elements-per-lane form, `dispatch_method` turns the method code into a template
// argument and `launch_lanes` launches. A kernel owns its model, its state type, how it addresses the noise field and (the
// affine kernel) the in-place advance.

// The twelve arguments every kernel takes -- `ys, y0, rows, cells, out_step, out_w, n, d, n_steps, n_out, key, key_dev` of
// TrajArgs, ExprArgs and ProgArgs -- filled from one place. Each block declares them where it always had them: a kernel's
// argument offsets decide how the compiler groups its scalar loads, and moving the fields into one leading sub-block changed
// the instruction count of 224 of this file's 246 kernels (profiles/traj_skeleton_resource_usage_notes.txt). The helpers
// below therefore take any of the three blocks.
template <typename T, typename Args>
static void traj_common(Args& p, void* ys, const void* y0, int64_t rows, int64_t d, const tsde_traj_t* tr, NoiseKey key,
                        const uint64_t* key_dev) {
  p.ys = (T*)ys;
  p.y0 = (const T*)y0;
  p.rows = (const T*)tr->step_rows;
  p.cells = tr->cells;
  p.out_step = tr->out_step;
  p.out_w = (const T*)tr->out_w;
  p.n = rows * d;
  p.d = d;
  p.n_steps = tr->n_steps;
  p.n_out = tr->n_out;
  p.key = key;
  p.key_dev = key_dev;
}

// Below this many 16-byte groups the one-element-per-lane form is used even when the vector form is legal:
// the kernel is ALU/latency bound per lane, so a half-empty chip finishes sooner with 4x the lanes.
constexpr int64_t kTrajVecMinGroups = 256 * 8 * 64;

// May a lane own 4 consecutive elements? Rows of whole 16-byte groups, the state and every `extra` table of the family
// aligned to them (a null pointer counts as aligned), and enough groups. What a family's noise addressing or coefficient
// tables demand on top, the family adds itself.
template <typename Args, typename... P>
static bool may_vec(const Args& c, const P*... extra) {
  return (c.d % 4 == 0) && aligned16(c.ys) && aligned16(c.y0) && (aligned16(extra) && ...) &&
         ((c.n * sizeof(*c.ys)) % 16 == 0) && (c.n >> 2) >= kTrajVecMinGroups;
}

template <typename Args>
static bool nothing_to_do(const Args& c) { return c.n <= 0 || c.n_steps <= 0; }

// One lane per W elements: `lanes` of them in blocks of kBlock.
template <typename Args>
static hipError_t launch_lanes(void (*kernel)(const Args), int64_t lanes, hipStream_t s, const Args& args) {
  hipLaunchKernelGGL(kernel, dim3((unsigned)((lanes + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, args);
  return hipGetLastError();
}

template <typename T>
struct TrajArgs {
  T* ys;                    // (n_out, n) outputs after t0
  T* sens;                  // (n_out, kSens, n) sensitivities of those outputs, or nullptr
  const T* y0;              // (n)
  const T *a, *b, *c, *e;   // (d) per-channel coefficients -- or (n_steps, d) tables when `cstride` = d (TIMED kernels)
  int64_t cstride;          // elements between the coefficient rows of consecutive steps; 0: the same at every step
  const T* rows;            // (n_steps, 8): dt, dt/2, 1/dt, sqrt(dt), sqrt(h), sqrt(h/12), h, 0
  const uint32_t* cells;    // (n_steps)
  const int32_t* out_step;  // (n_out) ascending: output j is due once `out_step[j]` steps are complete
  const T* out_w;           // (n_out, 2) weights on (previous state, current state)
  int64_t n, d;
  int32_t n_steps, n_out;
  NoiseKey key;
  const uint64_t* key_dev;
  uint32_t flags;           // TSDE_TRAJ_PACE_WAVES of `tsde_traj_t.flags` (appended: read by the paced forms only)
#ifdef TSDE_WAVE_STAMPS
  uint64_t* stamps;         // (waves, 4): start, end, HW_ID | XCC_ID << 32, 0 -- the diagnostic build only
#endif
};

enum : int { kEuler = TSDE_TRAJ_EULER, kMilIto = TSDE_TRAJ_MILSTEIN_ITO, kMilStrat = TSDE_TRAJ_MILSTEIN_STRAT,
             kMidpoint = TSDE_TRAJ_MIDPOINT, kSrk = TSDE_TRAJ_SRK, kHeun = TSDE_TRAJ_HEUN, kEulerHeun = TSDE_TRAJ_EULER_HEUN };

// The method code as a template argument: `fn(std::integral_constant<int, kEuler>{})` ...
template <typename F>
static hipError_t dispatch_method(int method, F fn) {
  switch (method) {
    case kEuler: return fn(std::integral_constant<int, kEuler>{});
    case kMilIto: return fn(std::integral_constant<int, kMilIto>{});
    case kMilStrat: return fn(std::integral_constant<int, kMilStrat>{});
    case kMidpoint: return fn(std::integral_constant<int, kMidpoint>{});
    case kSrk: return fn(std::integral_constant<int, kSrk>{});
    case kHeun: return fn(std::integral_constant<int, kHeun>{});
    case kEulerHeun: return fn(std::integral_constant<int, kEulerHeun>{});
    default: return hipErrorInvalidValue;
  }
}

// One step of one element of a diagonal SDE whose drift and diffusion the kernel can evaluate itself. `w` = W, `u` = U
// (SRK only). S is T (values only) or Dual<T>. `M` supplies f(x), g(x) and gdg(x, g, v) = (g * v) * g'(x), the
// diffusion VJP with cotangent g * v that derivative-form Milstein takes through autograd (base_sde.py:147-152).
// Stage-time slots. A scheme evaluates f and g at a few times of the step; a model whose coefficients depend on t holds
// one coefficient set per slot (TIMED kernels) and `m.f<SLOT>(x)` picks it; models with constant coefficients ignore the slot.
//   Euler, Milstein : slot 0 = t0                                         (euler.py:31, milstein.py:54)
//   midpoint        : slot 0 = t0, 1 = t0 + dt/2                          (midpoint.py:33,40)
//   SRK (SRID2)     : slot 0 = t0, 1 = t0 + dt/4, 2 = t0 + dt/2, 3 = t0 + dt;  f at C0 = (0, 1, 1/2) -> slots 0, 3, 2 and
//                     g at C1 = (0, 1/4, 1, 1/4) -> slots 0, 1, 3, 1       (srk.py:66-72, tableaus/srid2.py:21-22)
//   Heun, Euler-Heun: slot 0 = t0, 1 = t0 + dt = t1                       (heun.py:39,43, euler_heun.py:33,37)
template <int METHOD>
constexpr int stage_slots() {
  return METHOD == kSrk ? 4 : ((METHOD == kMidpoint || METHOD == kHeun || METHOD == kEulerHeun) ? 2 : 1);
}

template <typename T, int METHOD, typename S, typename M, typename N = T>
TSDE_D S scheme_step(const S y, const M& m, const N w, const N u, const T dt, const T half_dt, const T rdt,
                     const T sqrt_dt) {
  if constexpr (METHOD == kEuler) {
    return drift_diffusion_update<T, S>(y, m.template f<0>(y), m.template g<0>(y), w, dt, (T)1);
  } else if constexpr (METHOD == kMilIto || METHOD == kMilStrat) {
    const N v2 = milstein_v<T>(w, dt, (T)0.5, METHOD == kMilIto);
    const S g = m.template g<0>(y);
    const S gdg = m.template gdg<0>(y, g, v2);
    return milstein_update<T, S>(y, m.template f<0>(y), g, gdg, w, dt);
  } else if constexpr (METHOD == kMidpoint) {
    const S yp = drift_diffusion_update<T, S>(y, m.template f<0>(y), m.template g<0>(y), w, half_dt, (T)0.5);
    return drift_diffusion_update<T, S>(y, m.template f<1>(yp), m.template g<1>(yp), w, dt, (T)1);
  } else if constexpr (METHOD == kHeun || METHOD == kEulerHeun) {
    // Stratonovich predictor-corrector (heun.py:35-48, euler_heun.py:29-42) in the operation order of the stepwise route
    // (tsde_step_diag as predictor, tsde_heun_final): Heun predicts with the full Euler step, Euler-Heun with the noise alone
    constexpr bool heun = METHOD == kHeun;
    const S f0 = m.template f<0>(y), g0 = m.template g<0>(y);
    const S yp = drift_diffusion_update<T, S>(y, f0, g0, w, heun ? dt : (T)0, (T)1);
    const S g1 = m.template g<1>(yp);
    const S p0 = g0 * w, p1 = g1 * w;
    if constexpr (heun) {
      const S f1 = m.template f<1>(yp);
      return y + (((dt * (f0 + f1)) + p0) + p1) * (T)0.5;
    } else {
      return (y + dt * f0) + ((p0 + p1) * (T)0.5);
    }
  } else {
    const S zero = S((T)0);
    S f[3], g[4], h0, h1;
    S fz[3] = {zero, zero, zero};
    f[0] = m.template f<0>(y);
    g[0] = m.template g<0>(y);
    fz[0] = Srid2::need_f(1, 0) ? f[0] : zero;
    srid2_stage_states<T, 1, S>(y, fz, g, u, dt, rdt, sqrt_dt, h0, h1);
    f[1] = m.template f<3>(h0);
    g[1] = m.template g<1>(h1);
    fz[0] = Srid2::need_f(2, 0) ? f[0] : zero;
    fz[1] = Srid2::need_f(2, 1) ? f[1] : zero;
    srid2_stage_states<T, 2, S>(y, fz, g, u, dt, rdt, sqrt_dt, h0, h1);
    f[2] = m.template f<2>(h0);
    g[2] = m.template g<3>(h1);
    fz[0] = Srid2::need_f(3, 0) ? f[0] : zero;
    fz[1] = Srid2::need_f(3, 1) ? f[1] : zero;
    fz[2] = Srid2::need_f(3, 2) ? f[2] : zero;
    srid2_stage_states<T, 3, S>(y, fz, g, u, dt, rdt, sqrt_dt, h0, h1);
    g[3] = m.template g<1>(h1);
    return srid2_final<T, S>(y, f, g, w, u, dt, rdt, sqrt_dt);
  }
}

// The Euler and midpoint steps of `scheme_step` on steps whose dt and sqrt(h) are powers of two (TSDE_TRAJ_POW2_STEPS): `z`
// is the UNSCALED standard normal, `sw` = sqrt(h) and `half_sw` = sqrt(h)/2 (midpoint only). The same floats, bit for bit, in
// the domain `drift_diffusion_update_pow2` states. Values only.
template <typename T, int METHOD, typename M>
TSDE_D T scheme_step_pow2(const T y, const M& m, const T z, const T dt, const T half_dt, const T sw, const T half_sw) {
  static_assert(METHOD == kEuler || METHOD == kMidpoint, "the folded step exists for Euler and midpoint");
  if constexpr (METHOD == kEuler) {
    return drift_diffusion_update_pow2<T>(y, m.template f<0>(y), m.template g<0>(y), z, dt, sw);
  } else {
    const T yp = drift_diffusion_update_pow2<T>(y, m.template f<0>(y), m.template g<0>(y), z, half_dt, half_sw);
    return drift_diffusion_update_pow2<T>(y, m.template f<1>(yp), m.template g<1>(yp), z, dt, sw);
  }
}

// A shift that is zero by construction (the LINEAR form, f = a*x, g = c*x: geometric Brownian motion, any user module
// recognised as `mu * y`, `sigma * y`): it occupies no register and `x + NoShift{}` is x, no instruction. The stepwise
// route evaluates such a module with no addition at all; against `x + 0` the only difference is the sign of a zero.
struct NoShift {};
template <typename X>
TSDE_D X operator+(const X& x, NoShift) { return x; }

// Affine drift and diffusion, f = a*x + b, g = c*x + e; the coefficient types A..E are T or Seed<T, 1..4>, B and E also NoShift.
template <typename T, typename S, typename A, typename B, typename C, typename E>
struct AffineModel {
  A a;
  B b;
  C c;
  E e;
  template <int SLOT>
  TSDE_D S f(const S& x) const { return a * x + b; }
  template <int SLOT>
  TSDE_D S g(const S& x) const { return c * x + e; }
  template <int SLOT>
  TSDE_D S gdg(const S&, const S& gv, T v2) const { return (gv * v2) * c; }   // vjp of y -> c*y + e with cotangent g*v2
};

// ... with one coefficient set per stage-time slot (coefficients that depend on t; values only)
template <typename T, int NS>
struct AffineModelTimed {
  T a[NS], b[NS], c[NS], e[NS];
  template <int SLOT>
  TSDE_D T f(const T& x) const { return a[SLOT] * x + b[SLOT]; }
  template <int SLOT>
  TSDE_D T g(const T& x) const { return c[SLOT] * x + e[SLOT]; }
  template <int SLOT>
  TSDE_D T gdg(const T&, const T& gv, T v2) const { return (gv * v2) * c[SLOT]; }
};

template <typename T, int METHOD, typename S, typename A, typename B, typename C, typename E>
TSDE_D S affine_step(const S y, const A a, const B b, const C c, const E e, const T w, const T u, const T dt,
                     const T half_dt, const T rdt, const T sqrt_dt) {
  const AffineModel<T, S, A, B, C, E> m{a, b, c, e};
  return scheme_step<T, METHOD, S>(y, m, w, u, dt, half_dt, rdt, sqrt_dt);
}

// ---- elementwise expressions ------------------------------------------------------------------------------------------
// f = fa * phi_f(fp * x + fq) + fb and g = ga * phi_g(gp * x + gq) + gb per channel, phi from a fixed set
// (closed_form.py: ElementwiseDiagonalSDE). The function codes are uniform over the launch (scalar branches). The
// evaluation mirrors what torch computes for the module's f / g on the stepwise path, operation by operation
// (`scale * phi(rate * y + shift) + offset`; sigmoid as 1 / (1 + exp(-u)), softplus with torch's threshold 20).
template <typename T>
TSDE_D T expr_phi(int kind, T u) {
  switch (kind) {
    case TSDE_FN_EXP: return exp(u);
    case TSDE_FN_SIGMOID: return (T)1 / ((T)1 + exp(-u));
    case TSDE_FN_TANH: return tanh(u);
    case TSDE_FN_SOFTPLUS: return u > (T)20 ? u : log1p(exp(u));
    case TSDE_FN_SIN: return sin(u);
    case TSDE_FN_COS: return cos(u);
    default: return u;
  }
}

// phi'(u), given phi(u) = v where that is cheaper
template <typename T>
TSDE_D T expr_dphi(int kind, T u, T v) {
  switch (kind) {
    case TSDE_FN_EXP: return v;
    case TSDE_FN_SIGMOID: return v * ((T)1 - v);
    case TSDE_FN_TANH: return (T)1 - v * v;
    case TSDE_FN_SOFTPLUS: return u > (T)20 ? (T)1 : (T)1 / ((T)1 + exp(-u));
    case TSDE_FN_SIN: return cos(u);
    case TSDE_FN_COS: return -sin(u);
    default: return (T)1;
  }
}

template <typename T>
struct ExprModel {
  T fa, fp, fq, fb, ga, gp, gq, gb;
  int fk, gk;
  // kind TSDE_FN_POLY3: the four coefficients are those of a cubic, ((c3 x + c2) x + c1) x + c0 (a drift such as y - y^3,
  // logistic growth, a quadratic diffusion): sums and products of several affine functions of the state
  template <int SLOT>
  TSDE_D T f(const T& x) const {
    if (fk == TSDE_FN_POLY3) return ((fa * x + fp) * x + fq) * x + fb;
    return fa * expr_phi<T>(fk, fp * x + fq) + fb;
  }
  template <int SLOT>
  TSDE_D T g(const T& x) const {
    if (gk == TSDE_FN_POLY3) return ((ga * x + gp) * x + gq) * x + gb;
    return ga * expr_phi<T>(gk, gp * x + gq) + gb;
  }
  // (g v) g'(x), the chain rule in the order autograd walks scale * phi(rate * x + shift) + offset backwards
  template <int SLOT>
  TSDE_D T gdg(const T& x, const T& gv, T v2) const {
    if (gk == TSDE_FN_POLY3) return (gv * v2) * ((((T)3 * ga) * x + (T)2 * gp) * x + gq);
    const T u = gp * x + gq;
    return (((gv * v2) * ga) * expr_dphi<T>(gk, u, expr_phi<T>(gk, u))) * gp;
  }
};

// ... with one set of the eight coefficients per stage-time slot (coefficients that depend on t)
template <typename T, int NS>
struct ExprModelTimed {
  T k[NS][8];          // fa, fp, fq, fb, ga, gp, gq, gb
  int fk, gk;
  template <int SLOT>
  TSDE_D T f(const T& x) const {
    if (fk == TSDE_FN_POLY3) return ((k[SLOT][0] * x + k[SLOT][1]) * x + k[SLOT][2]) * x + k[SLOT][3];
    return k[SLOT][0] * expr_phi<T>(fk, k[SLOT][1] * x + k[SLOT][2]) + k[SLOT][3];
  }
  template <int SLOT>
  TSDE_D T g(const T& x) const {
    if (gk == TSDE_FN_POLY3) return ((k[SLOT][4] * x + k[SLOT][5]) * x + k[SLOT][6]) * x + k[SLOT][7];
    return k[SLOT][4] * expr_phi<T>(gk, k[SLOT][5] * x + k[SLOT][6]) + k[SLOT][7];
  }
  template <int SLOT>
  TSDE_D T gdg(const T& x, const T& gv, T v2) const {
    if (gk == TSDE_FN_POLY3) return (gv * v2) * ((((T)3 * k[SLOT][4]) * x + (T)2 * k[SLOT][5]) * x + k[SLOT][6]);
    const T u = k[SLOT][5] * x + k[SLOT][6];
    return (((gv * v2) * k[SLOT][4]) * expr_dphi<T>(gk, u, expr_phi<T>(gk, u))) * k[SLOT][5];
  }
};

template <typename T>
TSDE_D T primal(const T& x) { return x; }
template <typename T>
TSDE_D T primal(const Dual<T>& x) { return x.v; }

// ---- the step loop's shared pieces ------------------------------------------------------------------------------------
// Element i of one of a solve's host-written tables. UNIFORM: through the constant address space (`uniform_load`), as the
// affine kernel reads them; the other kernels read them plainly.
template <bool UNIFORM, typename X>
TSDE_D X table_read(const X* p, int64_t i) {
  if constexpr (UNIFORM) return uniform_load(p, i);
  else return p[i];
}

// Step count at which output j is due, as a wave-uniform (scalar) value; -1 past the last output.
template <bool UNIFORM>
TSDE_D int next_output_step(const int32_t* out_step, int j, int n_out) {
  if constexpr (UNIFORM) return j < n_out ? uniform_load(out_step, j) : -1;
  else return j < n_out ? __builtin_amdgcn_readfirstlane(out_step[j]) : -1;
}

// The scalars of step k (a row of `rows`: what a kernel does not use costs it nothing) and its Brownian cell. The eighth
// scalar, the time t0 the step starts at, is read on demand: only the program kernels use it, after their draws.
template <typename T>
struct StepRow {
  T dt, half_dt, rdt, sqrt_dt, sw, sh, th;
  uint32_t cell;
  const T* row;
  TSDE_D T t0() const { return row[7]; }
};

// `row`: the caller's `p.rows + (int64_t)k * 8` (wave-uniform: scalar loads); the TIMED kernels address their coefficient
// rows from the same k, and the address arithmetic stays theirs.
template <bool UNIFORM, typename T>
TSDE_D StepRow<T> step_row(const T* row, const uint32_t* cells, int k) {
  StepRow<T> r;
  r.dt = table_read<UNIFORM>(row, 0);
  r.half_dt = table_read<UNIFORM>(row, 1);
  r.rdt = table_read<UNIFORM>(row, 2);
  r.sqrt_dt = table_read<UNIFORM>(row, 3);
  r.sw = table_read<UNIFORM>(row, 4);
  r.sh = table_read<UNIFORM>(row, 5);
  r.th = table_read<UNIFORM>(row, 6);
  r.cell = table_read<UNIFORM>(cells, k);
  r.row = row;
  return r;
}

// W = z sqrt(h) and, NEED_U (SRK), U = h (W / 2 + z' sqrt(h / 12)) from standard normals z of stream W and z' of stream H,
// for the single element `elem`. !SCALED (the POW2 form of the affine kernel, whose step applies sqrt(h) itself): `w` = z.
template <typename T, bool NEED_U, bool SCALED = true, typename Noise>
TSDE_D void draw_one(const Noise& noise, const StepRow<T>& r, uint64_t elem, T& w, T& u) {
  static_assert(SCALED || !NEED_U, "U is made from the scaled W");
  const T z = noise.template normal1<T>(elem, kStreamW);
  w = SCALED ? z * r.sw : z;
  if constexpr (NEED_U) u = r.th * ((T)0.5 * w + noise.template normal1<T>(elem, kStreamH) * r.sh);
}

// The increments of a lane's W elements, the first of which meets element `elem` of the noise field; `u` is written only
// when NEED_U. W = 4: one Philox quad -- PAIRS: through `normal4_pairs` in place of `normal4`, the SRK form of the affine
// kernel, whose registers the shared series costs a wave (profiles/bm_shared_series_resource_usage_notes.txt). Otherwise
// element by element: one element per lane, or (W = d, a generated row model: specialise.py) a lane that owns a whole ROW
// of a small coupled system and draws its d increments one by one. `row_noise` (scalar noise): `elem` is the lane's row and
// all W elements meet its one increment. !SCALED: as `draw_one`, the unscaled normals on every path.
template <typename T, int W, bool NEED_U, bool PAIRS, bool SCALED = true, typename Noise>
TSDE_D void draw_increment(const Noise& noise, const StepRow<T>& r, uint64_t elem, bool row_noise, T (&w)[W], T (&u)[W]) {
  if (row_noise) {
    T w_row, u_row;
    draw_one<T, NEED_U, SCALED>(noise, r, elem, w_row, u_row);
#pragma unroll
    for (int q = 0; q < W; ++q) {
      w[q] = w_row;
      if constexpr (NEED_U) u[q] = u_row;
    }
  } else if constexpr (W == 4) {
    T z[4];
    if constexpr (PAIRS) noise.normal4_pairs(elem >> 2, kStreamW, z);
    else noise.normal4(elem >> 2, kStreamW, z);
#pragma unroll
    for (int q = 0; q < 4; ++q) w[q] = SCALED ? z[q] * r.sw : z[q];
    if constexpr (NEED_U) {
      if constexpr (PAIRS) noise.normal4_pairs(elem >> 2, kStreamH, z);
      else noise.normal4(elem >> 2, kStreamH, z);
#pragma unroll
      for (int q = 0; q < 4; ++q) u[q] = r.th * ((T)0.5 * w[q] + z[q] * r.sh);
    }
  } else {
#pragma unroll
    for (int q = 0; q < W; ++q) draw_one<T, NEED_U, SCALED>(noise, r, elem + (uint64_t)q, w[q], u[q]);
  }
}

// The outputs due once step k is complete: the cold block of the loop, entered when `k + 1 == next_out` (the step count of
// the next output lives in a scalar register: a step that is not an output time -- all but a few of them -- pays one scalar
// compare). `p`: the kernel's argument block; `y_old`, `y_new`: the lane's W elements (from index i) at the start and at the end
// of the step -- an output time inside the step interpolates between them. Advances `j` past the outputs written and `next_out`
// to the step count of the next one. Values only: the two sites whose state is a dual number (the SENS form of the affine
// kernel, `trajectory_prog_sens_kernel`) keep this block written out with their tangent planes -- through a function their
// register allocation came out wider, a wave of occupancy for the float64 forms.
template <bool UNIFORM, int W, typename Args, typename T>
TSDE_D void emit_outputs(const Args& p, int64_t i, int k, int& j, int& next_out, const T* y_old, const T* y_new) {
  if (!__builtin_expect(k + 1 == next_out, 0)) return;
  while (j < p.n_out && table_read<UNIFORM>(p.out_step, j) == k + 1) {
    const T w0 = table_read<UNIFORM>(p.out_w, 2 * j), w1 = table_read<UNIFORM>(p.out_w, 2 * j + 1);
    const bool exact = (w0 == (T)0 && w1 == (T)1);
    Pack<T, W> ov;
#pragma unroll
    for (int q = 0; q < W; ++q) ov.v[q] = exact ? y_new[q] : (w0 * y_old[q] + w1 * y_new[q]);
    store<T, W>(p.ys + (int64_t)j * p.n, i, ov);
    ++j;
  }
  next_out = next_output_step<UNIFORM>(p.out_step, j, p.n_out);
}

// What the affine kernel's step k takes from the solve's tables: its row, and the uniform head of its Philox calls.
template <typename T>
struct StepData {
  StepRow<T> r;
  StepNoise noise;
};

template <typename T>
TSDE_D StepData<T> step_data(const TrajArgs<T>& p, const NoiseKey& key, int k) {
  const StepRow<T> r = step_row<true>(p.rows + (int64_t)k * 8, p.cells, k);
  return {r, StepNoise(key, r.cell)};
}

// The forms of the affine kernel whose loop is rotated by one step: the scalar loads of step k + 1 (its row and its cell)
// are issued during step k and carried across the back edge in scalar registers, so that the one `s_waitcnt` left stands at
// the latch, a whole step after the loads, and the top of a step -- the Philox head, four scalar operations that every
// vector instruction of the step depends on -- no longer waits for the scalar cache with nothing else to issue. Chosen per
// form by the compiled loop (no vector register, no vector instruction, no scratch more than the plain loop) and by the
// device: Euler, both Milsteins, Heun and Euler-Heun, float32, one 16-byte group per lane, constant coefficients. Midpoint
// measured slower rotated and SRK, whose loop waits for its loads where it uses them either way, the same; the TIMED forms
// gain vector instructions; W = 1, float64 and SENS were not measured (profiles/step_ahead_notes.txt). Those keep the
// plain loop.
template <typename T, int METHOD, int W, bool SENS, bool TIMED>
constexpr bool step_ahead_form() {
  return std::is_same<T, float>::value && W == 4 && !SENS && !TIMED && METHOD != kMidpoint && METHOD != kSrk;
}

#ifdef TSDE_WAVE_STAMPS
// The diagnostic build of tools/wave_finish_times.hip: when a wave started and ended on the 100 MHz clock and where it ran
// (HW_ID: SIMD, CU, SE; XCC_ID), one vector store by the wave's first active lane into a buffer nothing else reads. The
// shipped library is built without the macro and holds no stamp.
struct WaveStamp {
  uint64_t t0;
  TSDE_D WaveStamp() : t0(__builtin_amdgcn_s_memrealtime()) {}
  TSDE_D void store(uint64_t* out) const {
    const uint64_t t1 = __builtin_amdgcn_s_memrealtime();
    const uint32_t hw = __builtin_amdgcn_s_getreg(4 | (31 << 11)), xcc = __builtin_amdgcn_s_getreg(20 | (31 << 11));
    const int lane = threadIdx.x & 63;
    if (lane != __builtin_amdgcn_readfirstlane(lane)) return;
    const int64_t wave = (int64_t)blockIdx.x * (kBlock / 64) + threadIdx.x / 64;
    typedef uint64_t u64x4 __attribute__((ext_vector_type(4)));
    const u64x4 v = {t0, t1, (uint64_t)hw | ((uint64_t)xcc << 32), 0};
    *reinterpret_cast<u64x4*>(out + wave * 4) = v;
  }
};
#endif

// The forms of the affine kernel whose waves pace themselves (`wave_pace`, tsde_common.h) when the schedule carries
// TSDE_TRAJ_PACE_WAVES: the loop carries the step count of the next change of priority in a scalar register, as it carries
// `next_out`, and pays one scalar compare per step; a change is a cold block. Chosen per form by the compiled loop (the vector
// instructions, vector registers and scratch of the plain loop) and by the device (profiles/wave_pacing_ab.json): Euler,
// midpoint and Heun, float32, one 16-byte group per lane, constant coefficients. Milstein (Ito) and SRK measured SLOWER paced
// and keep the plain loop; Stratonovich Milstein, Euler-Heun, float64, W = 1, SENS and TIMED were not measured and are not paced.
template <typename T, int METHOD, int W, bool SENS, bool TIMED>
constexpr bool wave_paced_form() {
  return std::is_same<T, float>::value && W == 4 && !SENS && !TIMED &&
         (METHOD == kEuler || METHOD == kMidpoint || METHOD == kHeun);
}

// W = 4: a lane owns one 16-byte group (needs d % 4 == 0 so the group stays inside one row).
// W = 1: a lane owns one element (any d; also used for small problems, where it exposes 4x the lanes).
// SENS : carry the kSens path-wise sensitivities of every element and write them next to the outputs.
// TIMED: the coefficients are functions of time, f(t, y) = a(t) * y + b(t), given as one row per STAGE TIME of every step
//        (`stage_slots<METHOD>()` rows per step, in slot order): re-read, through the L2, at the top of every step. A
//        separate instantiation, so the constant-coefficient kernels are untouched.
// LINEAR: both shifts are zero (`p.b`, `p.e` are null and never read): f = a*y, g = c*y. Chosen by the host, values only,
//        constant coefficients only -- the sensitivity kernels carry d/db and d/de, which are live at a zero shift too.
// POW2:  every step's dt and sqrt(h) are powers of two (the schedule's TSDE_TRAJ_POW2_STEPS: the host looked at the rows, the
//        launcher chooses). The draw hands out the unscaled normals and the step folds both scalings into fused multiply-adds
//        (`scheme_step_pow2`): 4 multiplies and 2 fmas per element of an Euler step in place of 6 multiplies and 2 adds. Bit
//        for bit the plain form's floats unless a product f*dt or g*z*sqrt(h) is subnormal -- |a*y| or |c*y| below about
//        2^-126 / (|z| sqrt(h)) -- where this form rounds once fewer (a few units in the last place of a state that small);
//        no per-element guard, which would cost more than the fold saves. Euler and midpoint, float32, values only, constant
//        coefficients; with or without shifts. Milstein, Heun, Euler-Heun and float64 have no folded step yet.
template <typename T, int METHOD, int W, bool SENS, bool TIMED = false, bool LINEAR = false, bool POW2 = false>
__global__ void __launch_bounds__(kBlock) trajectory_kernel(const TrajArgs<T> p) {
  static_assert(!LINEAR || (!SENS && !TIMED), "the linear form: values only, constant coefficients");
  static_assert(!POW2 || (!SENS && !TIMED && (METHOD == kEuler || METHOD == kMidpoint)),
                "the folded step: Euler and midpoint, values only, constant coefficients");
  constexpr bool kNeedU = METHOD == kSrk;
  constexpr bool kInPlace = !SENS && !TIMED;
  using S = typename std::conditional<SENS, Dual<T>, T>::type;
  using A = typename std::conditional<SENS, Seed<T, 1>, T>::type;
  using B = typename std::conditional<LINEAR, NoShift, typename std::conditional<SENS, Seed<T, 2>, T>::type>::type;
  using C = typename std::conditional<SENS, Seed<T, 3>, T>::type;
  using E = typename std::conditional<LINEAR, NoShift, typename std::conditional<SENS, Seed<T, 4>, T>::type>::type;
  const int64_t lane = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t i = lane * W;
  if (i >= p.n) return;
#ifdef TSDE_WAVE_STAMPS
  const WaveStamp stamp;
#endif
  const int64_t col = i % p.d;
  const Pack<T, W> a = load<T, W>(p.a, col), c = load<T, W>(p.c, col);
  Pack<T, W> b, e;
  if constexpr (!LINEAR) {
    b = load<T, W>(p.b, col);
    e = load<T, W>(p.e, col);
  }
  const Pack<T, W> y_init = load<T, W>(p.y0, i);
  S y[W], y_prev[W];  // the state; and the state at the start of a step that meets an output time
#pragma unroll
  for (int q = 0; q < W; ++q) {
    y[q] = y_prev[q] = S(y_init.v[q]);
    if constexpr (SENS) y[q].d[0] = (T)1;
  }
  NoiseKey key = p.key;
  if (p.key_dev != nullptr) {
    const uint64_t ent = uniform_load(p.key_dev, 0);
    key.k0 = (uint32_t)ent;
    key.k1 = (uint32_t)(ent >> 32);
  }
  const uint64_t elem = key.elem0 + (uint64_t)i;
  int j = 0;
  int next_out = next_output_step<true>(p.out_step, 0, p.n_out);
  constexpr bool kAhead = step_ahead_form<T, METHOD, W, SENS, TIMED>();
  constexpr bool kPaced = wave_paced_form<T, METHOD, W, SENS, TIMED>();
  const WavePace pace = wave_pace(p.n_steps);
  int next_pace = -1;                               // (kPaced only: the step count of the wave's next change of priority)
  if constexpr (kPaced) {
    next_pace = wave_pace_first(pace, (p.flags & TSDE_TRAJ_PACE_WAVES) != 0);
    if (next_pace >= 0) {
      int level = 3;
      if (next_pace == 0) next_pace = wave_pace_change(pace, 0, level);   // (fewer than 2 steps: a change due at once)
      set_wave_priority(level);
    }
  }
  StepData<T> ahead = step_data(p, key, 0);         // (kAhead only: dead code, and removed, in the other forms)
  for (int k = 0; k < p.n_steps; ++k) {
    const StepData<T> now = ahead;                  // (kAhead: what step k - 1 loaded)
    const StepRow<T> r = kAhead ? now.r : step_row<true>(p.rows + (int64_t)k * 8, p.cells, k);
    if constexpr (kAhead) {
      const int kn = k + 1 < p.n_steps ? k + 1 : k;  // (clamped, never branched on: the last step re-reads its own row)
      ahead = step_data(p, key, kn);
    }
    constexpr int NS = stage_slots<METHOD>();
    Pack<T, W> ta[NS], tb[NS], tc[NS], te[NS];      // TIMED: the coefficient rows of this step's stage times
    if constexpr (TIMED) {
#pragma unroll
      for (int sl = 0; sl < NS; ++sl) {
        const int64_t at = ((int64_t)k * NS + sl) * p.cstride + col;
        ta[sl] = load<T, W>(p.a, at);
        tb[sl] = load<T, W>(p.b, at);
        tc[sl] = load<T, W>(p.c, at);
        te[sl] = load<T, W>(p.e, at);
      }
    }
    const StepNoise noise = kAhead ? now.noise : StepNoise(key, r.cell);   // (the uniform head of this step's Philox calls: scalar unit)
    Pack<T, W> w, u;
    draw_increment<T, W, kNeedU, /*PAIRS=*/kNeedU, /*SCALED=*/!POW2>(noise, r, elem, false, w.v, u.v);   // (SRK: the shared series costs it a wave)
    // Values-only kernels with constant coefficients advance the state IN PLACE: a step that ends at or after an output
    // time -- all but a few do not -- first sets the state it starts from aside (the interpolation inside a step needs both
    // ends) in a cold block, and the hot loop has no register copies at its latch. The others (dual numbers, coefficient
    // rows: wide states, where the copy's registers cost occupancy) keep both states and copy at the latch.
    const bool due = k + 1 == next_out;   // (also what `emit_outputs` tests after the step)
    S y1[W];
    if constexpr (kInPlace) {
      if (__builtin_expect(due, 0)) {
        asm volatile("" ::: "memory");    // (keeps this a branch: as selects it would cost W vector instructions per step)
#pragma unroll
        for (int q = 0; q < W; ++q) y_prev[q] = y[q];
      }
    }
    S* const y_new = kInPlace ? y : y1;
    const S* const y_old = kInPlace ? y_prev : y;
#pragma unroll
    for (int q = 0; q < W; ++q) {
      if constexpr (TIMED) {
        AffineModelTimed<T, NS> m;
#pragma unroll
        for (int sl = 0; sl < NS; ++sl) {
          m.a[sl] = ta[sl].v[q];
          m.b[sl] = tb[sl].v[q];
          m.c[sl] = tc[sl].v[q];
          m.e[sl] = te[sl].v[q];
        }
        y_new[q] = scheme_step<T, METHOD, S>(y[q], m, w.v[q], kNeedU ? u.v[q] : (T)0, r.dt, r.half_dt, r.rdt, r.sqrt_dt);
      } else {
        B bq;
        E eq;
        if constexpr (!LINEAR) {
          bq = B{b.v[q]};
          eq = E{e.v[q]};
        }
        if constexpr (POW2) {
          const AffineModel<T, S, A, B, C, E> m{A{a.v[q]}, bq, C{c.v[q]}, eq};
          y_new[q] = scheme_step_pow2<T, METHOD>(y[q], m, w.v[q], r.dt, r.half_dt, r.sw,
                                                 METHOD == kMidpoint ? half_of_pow2(r.sw) : r.sw);
        } else {
          y_new[q] = affine_step<T, METHOD, S, A, B, C, E>(y[q], A{a.v[q]}, bq, C{c.v[q]}, eq, w.v[q],
                                                            kNeedU ? u.v[q] : (T)0, r.dt, r.half_dt, r.rdt, r.sqrt_dt);
        }
      }
    }
    if constexpr (SENS) {
      if (__builtin_expect(due, 0)) {
        while (j < p.n_out && uniform_load(p.out_step, j) == k + 1) {
          const T w0 = uniform_load(p.out_w, 2 * j), w1 = uniform_load(p.out_w, 2 * j + 1);
          const bool exact = (w0 == (T)0 && w1 == (T)1);
          S o[W];
#pragma unroll
          for (int q = 0; q < W; ++q) o[q] = exact ? y_new[q] : (w0 * y_old[q] + w1 * y_new[q]);
          Pack<T, W> ov;
#pragma unroll
          for (int q = 0; q < W; ++q) ov.v[q] = primal<T>(o[q]);
          store<T, W>(p.ys + (int64_t)j * p.n, i, ov);
#pragma unroll
          for (int s = 0; s < kSens; ++s) {
#pragma unroll
            for (int q = 0; q < W; ++q) ov.v[q] = o[q].d[s];
            store<T, W>(p.sens + ((int64_t)j * kSens + s) * p.n, i, ov);
          }
          ++j;
        }
        next_out = next_output_step<true>(p.out_step, j, p.n_out);
      }
    } else {
      emit_outputs<true, W>(p, i, k, j, next_out, y_old, y_new);   // (tests `due` itself: next_out is unchanged since)
    }
    if constexpr (!kInPlace) {
#pragma unroll
      for (int q = 0; q < W; ++q) y[q] = y1[q];
    }
    if constexpr (kPaced) {                         // (at the latch, where the `due` test stands: the loop's top stays as it was)
      if (__builtin_expect(k + 1 == next_pace, 0)) {
        asm volatile("" ::: "memory");              // (keeps this a branch, like the `due` block)
        int level;
        next_pace = wave_pace_change(pace, k + 1, level);
        set_wave_priority(level);
      }
    }
  }
#ifdef TSDE_WAVE_STAMPS
  stamp.store(p.stamps);
#endif
}

template <typename T, int METHOD, bool SENS, bool TIMED = false, bool LINEAR = false, bool POW2 = false>
static hipError_t launch_traj_form(const TrajArgs<T>& p, bool vec, hipStream_t s) {
  if (vec) return launch_lanes(trajectory_kernel<T, METHOD, 4, SENS, TIMED, LINEAR, POW2>, p.n >> 2, s, p);
  return launch_lanes(trajectory_kernel<T, METHOD, 1, SENS, TIMED, LINEAR, POW2>, p.n, s, p);
}

// The values-only forms with constant coefficients; `pow2`: the schedule vouches for TSDE_TRAJ_POW2_STEPS. The folded step
// is built for float32 Euler and midpoint; everything else runs the plain form whatever the flag says.
template <typename T, int METHOD, bool LINEAR>
static hipError_t launch_traj_values(const TrajArgs<T>& p, bool vec, bool pow2, hipStream_t s) {
  if constexpr (std::is_same<T, float>::value && (METHOD == kEuler || METHOD == kMidpoint)) {
    if (pow2) return launch_traj_form<T, METHOD, false, false, LINEAR, true>(p, vec, s);
  }
  return launch_traj_form<T, METHOD, false, false, LINEAR>(p, vec, s);
}

template <typename T, int METHOD>
static hipError_t launch_traj_m(const TrajArgs<T>& p, bool vec, bool pow2, hipStream_t s) {
  if (p.cstride != 0) {            // coefficient tables (values only)
    if (p.sens) return hipErrorNotSupported;
    return launch_traj_form<T, METHOD, false, true>(p, vec, s);
  }
  if (p.b == nullptr && p.e == nullptr) {   // both shifts zero: the linear form (values only)
    if (p.sens) return hipErrorNotSupported;
    return launch_traj_values<T, METHOD, true>(p, vec, pow2, s);
  }
  return p.sens ? launch_traj_form<T, METHOD, true>(p, vec, s) : launch_traj_values<T, METHOD, false>(p, vec, pow2, s);
}

// (The four launchers of this file that the C entry points call dispatch on the dtype like the stepwise ones, tsde_launch.h:
//  by_dtype. A specialised unit includes this file for its helpers and kernels only and leaves them out.)
#ifndef TSDE_SPECIALISE_TU
hipError_t launch_trajectory_affine_diag(int dtype, void* ys, void* sens, const void* y0, int64_t rows, int64_t d,
                                         const void* a, const void* b, const void* c, const void* e, int64_t cstride,
                                         int method, const tsde_traj_t* tr, NoiseKey key, const uint64_t* key_dev,
                                         hipStream_t s) {
  return by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    TrajArgs<T> p;
    traj_common<T>(p, ys, y0, rows, d, tr, key, key_dev);
    p.sens = (T*)sens;
    p.a = (const T*)a;
    p.b = (const T*)b;
    p.c = (const T*)c;
    p.e = (const T*)e;
    p.cstride = cstride;
    p.flags = tr->flags;
    if ((b == nullptr) != (e == nullptr)) return hipErrorInvalidValue;   // the linear form takes BOTH shifts as null
    if (b == nullptr && (cstride != 0 || sens)) return hipErrorInvalidValue;
    if (nothing_to_do(p)) return hipSuccess;
    const bool vec = may_vec(p, p.a, p.b, p.c, p.e, p.sens) &&
                     (key.elem0 % 4 == 0) &&   // diagonal noise: a lane's 4 elements are one Philox quad
                     (cstride % 4 == 0);       // coefficient tables: every row starts on a 16-byte group
    const bool pow2 = (tr->flags & TSDE_TRAJ_POW2_STEPS) != 0;
    return dispatch_method(method, [&](auto m) { return launch_traj_m<T, decltype(m)::value>(p, vec, pow2, s); });
  });
}
#endif

template <typename T>
struct ExprArgs {
  T* ys;                    // (n_out, n) outputs after t0
  const T* y0;              // (n)
  const T* coef[8];         // (d) each: drift scale, rate, shift, offset; diffusion scale, rate, shift, offset
  int64_t cstride;          // as TrajArgs::cstride: (n_steps, d) tables for coefficients that depend on t
  int32_t f_kind, g_kind;
  const T* rows;
  const uint32_t* cells;
  const int32_t* out_step;
  const T* out_w;
  int64_t n, d;
  int32_t n_steps, n_out;
  NoiseKey key;
  const uint64_t* key_dev;
};

// The affine trajectory kernel's loop with the expression model in place of the affine one (values only).
template <typename T, int METHOD, int W, bool TIMED = false>
__global__ void __launch_bounds__(kBlock) trajectory_expr_kernel(const ExprArgs<T> p) {
  constexpr bool kNeedU = METHOD == kSrk;
  const int64_t lane = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t i = lane * W;
  if (i >= p.n) return;
  const int64_t col = i % p.d;
  Pack<T, W> cf[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) cf[c] = load<T, W>(p.coef[c], col);
  const Pack<T, W> y_init = load<T, W>(p.y0, i);
  T y[W];
#pragma unroll
  for (int q = 0; q < W; ++q) y[q] = y_init.v[q];
  const NoiseKey key = launch_key(p.key, p.key_dev);
  const uint64_t elem = key.elem0 + (uint64_t)i;
  int j = 0;
  int next_out = next_output_step<false>(p.out_step, 0, p.n_out);
  for (int k = 0; k < p.n_steps; ++k) {
    const StepRow<T> r = step_row<false>(p.rows + (int64_t)k * 8, p.cells, k);
    constexpr int NS = stage_slots<METHOD>();
    Pack<T, W> tcf[NS][8];                          // TIMED: the coefficient rows of this step's stage times
    if constexpr (TIMED) {
#pragma unroll
      for (int sl = 0; sl < NS; ++sl) {
        const int64_t at = ((int64_t)k * NS + sl) * p.cstride + col;
#pragma unroll
        for (int c = 0; c < 8; ++c) tcf[sl][c] = load<T, W>(p.coef[c], at);
      }
    }
    Pack<T, W> w, u;
    draw_increment<T, W, kNeedU, /*PAIRS=*/false>(PlainStepNoise(key, r.cell), r, elem, false, w.v, u.v);
    T y1[W];
#pragma unroll
    for (int q = 0; q < W; ++q) {
      if constexpr (TIMED) {
        ExprModelTimed<T, NS> m;
#pragma unroll
        for (int sl = 0; sl < NS; ++sl) {
#pragma unroll
          for (int c = 0; c < 8; ++c) m.k[sl][c] = tcf[sl][c].v[q];
        }
        m.fk = p.f_kind;
        m.gk = p.g_kind;
        y1[q] = scheme_step<T, METHOD, T>(y[q], m, w.v[q], kNeedU ? u.v[q] : (T)0, r.dt, r.half_dt, r.rdt, r.sqrt_dt);
      } else {
        const ExprModel<T> m{cf[0].v[q], cf[1].v[q], cf[2].v[q], cf[3].v[q], cf[4].v[q], cf[5].v[q],
                             cf[6].v[q], cf[7].v[q], p.f_kind,  p.g_kind};
        y1[q] = scheme_step<T, METHOD, T>(y[q], m, w.v[q], kNeedU ? u.v[q] : (T)0, r.dt, r.half_dt, r.rdt, r.sqrt_dt);
      }
    }
    emit_outputs<false, W>(p, i, k, j, next_out, y, y1);
#pragma unroll
    for (int q = 0; q < W; ++q) y[q] = y1[q];
  }
}

template <typename T, int METHOD>
static hipError_t launch_expr_m(const ExprArgs<T>& p, bool vec, hipStream_t s) {
  if (p.cstride != 0) {
    // (SRK holds 4 slots x 8 coefficients per element: one element per lane keeps that in registers)
    if (vec && METHOD != kSrk) return launch_lanes(trajectory_expr_kernel<T, METHOD, 4, true>, p.n >> 2, s, p);
    return launch_lanes(trajectory_expr_kernel<T, METHOD, 1, true>, p.n, s, p);
  }
  if (vec) return launch_lanes(trajectory_expr_kernel<T, METHOD, 4>, p.n >> 2, s, p);
  return launch_lanes(trajectory_expr_kernel<T, METHOD, 1>, p.n, s, p);
}

#ifndef TSDE_SPECIALISE_TU
hipError_t launch_trajectory_expr_diag(int dtype, void* ys, const void* y0, int64_t rows, int64_t d, const void* const coef[8],
                                       int64_t cstride, int f_kind, int g_kind, int method, const tsde_traj_t* tr,
                                       NoiseKey key, const uint64_t* key_dev, hipStream_t s) {
  return by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    ExprArgs<T> p;
    traj_common<T>(p, ys, y0, rows, d, tr, key, key_dev);
    for (int c = 0; c < 8; ++c) p.coef[c] = (const T*)coef[c];
    p.cstride = cstride;
    p.f_kind = f_kind;
    p.g_kind = g_kind;
    if (nothing_to_do(p)) return hipSuccess;
    const bool vec = may_vec(p, p.coef[0], p.coef[1], p.coef[2], p.coef[3], p.coef[4], p.coef[5], p.coef[6], p.coef[7]) &&
                     (key.elem0 % 4 == 0) &&   // diagonal noise: a lane's 4 elements are one Philox quad
                     (cstride % 4 == 0);       // coefficient tables: every row starts on a 16-byte group
    return dispatch_method(method, [&](auto m) { return launch_expr_m<T, decltype(m)::value>(p, vec, s); });
  });
}
#endif

// ---- expression PROGRAMS ------------------------------------------------------------------------------------------------
// Drift, diffusion (and the diffusion's derivative, for Milstein) as small postfix programs over a four-deep value stack:
// whatever elementwise code a user's f and g consist of -- several functions of the state summed or multiplied
// (`-p**2 * sin(y) * cos(y)**3`, tests/problems.py:84-86; `tanh(y) + y`; y**4) -- which the single-function forms above
// cannot express. recognise.py builds the expression tree of the user's code while it runs on the probe, orders it so that
// four stack slots suffice, and hands over: `code` (32-bit words: opcode | source << 8 | constant row << 16) and a table of
// per-channel constants (n_const, d). One instruction = one torch operator of the user's code, evaluated in the same order
// and (for + - * /) with the same rounding; functions as in `expr_phi`. The instruction stream is wave-uniform: decoding it
// is scalar work, the vector unit sees one operation per instruction and element.
//   source: 0 = the value below the top of the stack (binary operators pop it), 1 = constant row k of this channel, 2 = the state,
//           3 = the time t at which the scheme evaluates the function (its stage time: t_k, t_k + dt/4, t_k + dt/2 or t_k + dt)
//   a binary operator computes  A op B  with A = top of stack, B = source  (R variants: B op A); source 0: A = the value
//   below the top, B = the top (R variants swapped), and the result replaces both
enum : uint32_t { kSrcStack = 0, kSrcConst = 1, kSrcState = 2, kSrcTime = 3 };
enum : uint32_t {
  kOpLoad = 0, kOpAdd, kOpSub, kOpRsub, kOpMul, kOpDiv, kOpRdiv,                       // take a source
  kOpNeg = 16, kOpExp, kOpLog, kOpSin, kOpCos, kOpTanh, kOpSigmoid, kOpSoftplus, kOpSqrt, kOpAbs, kOpRelu, kOpRecip,
  kOpSquare, kOpCube, kOpDup
};

// W elements processed together: one decoded instruction serves all of them.
template <typename T, int W>
struct Vec {
  T v[W];
  Vec() = default;
  TSDE_D explicit Vec(T s) {
#pragma unroll
    for (int q = 0; q < W; ++q) v[q] = s;
  }
};
#define TSDE_VEC_BINARY(OP)                                                                  \
  template <typename T, int W>                                                               \
  TSDE_D Vec<T, W> operator OP(const Vec<T, W>& a, const Vec<T, W>& b) {                     \
    Vec<T, W> r;                                                                             \
    _Pragma("unroll") for (int q = 0; q < W; ++q) r.v[q] = a.v[q] OP b.v[q];                 \
    return r;                                                                                \
  }                                                                                          \
  template <typename T, int W>                                                               \
  TSDE_D Vec<T, W> operator OP(const Vec<T, W>& a, T b) {                                    \
    Vec<T, W> r;                                                                             \
    _Pragma("unroll") for (int q = 0; q < W; ++q) r.v[q] = a.v[q] OP b;                      \
    return r;                                                                                \
  }                                                                                          \
  template <typename T, int W>                                                               \
  TSDE_D Vec<T, W> operator OP(T a, const Vec<T, W>& b) {                                    \
    Vec<T, W> r;                                                                             \
    _Pragma("unroll") for (int q = 0; q < W; ++q) r.v[q] = a OP b.v[q];                      \
    return r;                                                                                \
  }
TSDE_VEC_BINARY(+)
TSDE_VEC_BINARY(-)
TSDE_VEC_BINARY(*)
TSDE_VEC_BINARY(/)
#undef TSDE_VEC_BINARY

template <typename T, int W, typename F>
TSDE_D Vec<T, W> vmap(const Vec<T, W>& a, F fn) {
  Vec<T, W> r;
#pragma unroll
  for (int q = 0; q < W; ++q) r.v[q] = fn(a.v[q]);
  return r;
}

constexpr int kProgWords = 96;     // instruction words of f, g and g' together (they travel in the kernel arguments)
constexpr int kProgRegs = 8;       // constant rows kept in registers; rows beyond are read through the cache at each use

template <typename T>
struct ProgArgs;

template <typename T, int W>
struct ProgModel {
  using V = Vec<T, W>;
  TSDE_D void setup(const ProgArgs<T>& p, int64_t column);
  const uint32_t* code;            // f program, then g, then g': kernel arguments -> scalar loads, wave-uniform
  int f_len, g_len, dg_len;
  const T* consts;                 // (n_const, d)
  int64_t d, col;                  // channel of this lane's first element
  V creg[kProgRegs];               // this lane's entries of the first constant rows
  T tslot[4];                      // the scheme's stage times of the current step (slot order of `stage_slots`)

  TSDE_D V constant(uint32_t k) const {
    switch (k) {                   // (uniform: a scalar branch; a register array indexed by k would go through scratch)
      case 0: return creg[0];
      case 1: return creg[1];
      case 2: return creg[2];
      case 3: return creg[3];
      case 4: return creg[4];
      case 5: return creg[5];
      case 6: return creg[6];
      case 7: return creg[7];
      default: {
        V r;
        const Pack<T, W> pk = load<T, W>(consts, (int64_t)k * d + col);
#pragma unroll
        for (int q = 0; q < W; ++q) r.v[q] = pk.v[q];
        return r;
      }
    }
  }

  TSDE_D V run(const uint32_t* prog, int len, const V& x, const T time) const {
    V s0((T)0), s1((T)0), s2((T)0), s3((T)0);
    uint32_t fetched = prog[0];
    for (int pc = 0; pc < len; ++pc) {
      // (the next word is requested before this one executes: the scalar load's latency hides behind the vector work)
      const uint32_t ins = fetched;
      fetched = prog[pc + 1 < len ? pc + 1 : pc];
      const uint32_t op = ins & 0xFFu, src = (ins >> 8) & 0xFFu, k = ins >> 16;
      if (op < kOpNeg) {
        V a = s0, b;
        if (src == kSrcStack) {        // pop: the operands are the two top values
          b = s0;
          a = s1;
          s1 = s2;
          s2 = s3;
        } else if (src == kSrcConst) {
          b = constant(k);
        } else if (src == kSrcTime) {
          b = V(time);
        } else {
          b = x;
        }
        switch (op) {
          case kOpLoad:                // push the source (never the stack)
            s3 = s2;
            s2 = s1;
            s1 = s0;
            s0 = b;
            break;
          case kOpAdd: s0 = a + b; break;
          case kOpSub: s0 = a - b; break;
          case kOpRsub: s0 = b - a; break;
          case kOpMul: s0 = a * b; break;
          case kOpDiv: s0 = a / b; break;
          default: s0 = b / a; break;  // kOpRdiv
        }
      } else {
        switch (op) {
          case kOpNeg: s0 = vmap(s0, [](T v) { return -v; }); break;
          case kOpExp: s0 = vmap(s0, [](T v) { return exp(v); }); break;
          case kOpLog: s0 = vmap(s0, [](T v) { return log(v); }); break;
          case kOpSin: s0 = vmap(s0, [](T v) { return sin(v); }); break;
          case kOpCos: s0 = vmap(s0, [](T v) { return cos(v); }); break;
          case kOpTanh: s0 = vmap(s0, [](T v) { return tanh(v); }); break;
          case kOpSigmoid: s0 = vmap(s0, [](T v) { return (T)1 / ((T)1 + exp(-v)); }); break;
          case kOpSoftplus: s0 = vmap(s0, [](T v) { return v > (T)20 ? v : log1p(exp(v)); }); break;
          case kOpSqrt: s0 = vmap(s0, [](T v) { return sqrt(v); }); break;
          case kOpAbs: s0 = vmap(s0, [](T v) { return fabs(v); }); break;
          case kOpRelu: s0 = vmap(s0, [](T v) { return v > (T)0 ? v : (T)0; }); break;
          case kOpRecip: s0 = vmap(s0, [](T v) { return (T)1 / v; }); break;
          case kOpSquare: s0 = s0 * s0; break;
          case kOpCube: s0 = (s0 * s0) * s0; break;
          default:                     // kOpDup
            s3 = s2;
            s2 = s1;
            s1 = s0;
            break;
        }
      }
    }
    return s0;
  }
  template <int SLOT>
  TSDE_D V f(const V& x) const { return run(code, f_len, x, tslot[SLOT]); }
  template <int SLOT>
  TSDE_D V g(const V& x) const { return run(code + f_len, g_len, x, tslot[SLOT]); }
  template <int SLOT>
  TSDE_D V gdg(const V& x, const V& gv, const V& v2) const {
    return (gv * v2) * run(code + f_len + g_len, dg_len, x, tslot[SLOT]);
  }
};

// The times at which a scheme evaluates f and g within the step that starts at t0 (slot order of `stage_slots`; computed like
// the stepwise path's host code: t0 + frac * dt in the state dtype).
template <typename T, int METHOD>
TSDE_D void stage_times(T t0, T dt, T (&out)[4]) {
  out[0] = t0;
  out[1] = METHOD == kSrk ? t0 + (T)0.25 * dt : ((METHOD == kHeun || METHOD == kEulerHeun) ? t0 + dt : t0 + (T)0.5 * dt);
  out[2] = t0 + (T)0.5 * dt;
  out[3] = t0 + dt;
}

template <typename T>
struct ProgArgs {
  T* ys;
  const T* y0;
  const T* consts;
  int32_t f_len, g_len, dg_len, n_const;
  int32_t scalar_noise;     // 1: one Brownian channel per ROW (noise type "scalar"): element (row, c) meets increment `row`
  const T* rows;
  const uint32_t* cells;
  const int32_t* out_step;
  const T* out_w;
  int64_t n, d;
  int32_t n_steps, n_out;
  NoiseKey key;
  const uint64_t* key_dev;
  uint32_t code[kProgWords];
};

template <typename T, int W>
TSDE_D void ProgModel<T, W>::setup(const ProgArgs<T>& p, int64_t column) {
  code = p.code;
  f_len = p.f_len;
  g_len = p.g_len;
  dg_len = p.dg_len;
  consts = p.consts;
  d = p.d;
  col = column;
#pragma unroll
  for (int k = 0; k < kProgRegs; ++k) {
    creg[k] = V((T)0);
    if (k < p.n_const) {
      const Pack<T, W> pk = load<T, W>(p.consts, (int64_t)k * p.d + col);
#pragma unroll
      for (int q = 0; q < W; ++q) creg[k].v[q] = pk.v[q];
    }
  }
}

// The expression kernels' loop with the program model; a lane's W elements run through each program together.
// W = 4 needs d % 4 == 0 (a lane's elements share their row).
// `M`: the model of drift and diffusion -- `ProgModel` (the interpreter), or a struct GENERATED from the same programs and
// compiled at run time (torchsde_amd/specialise.py: the instruction stream becomes straight-line code, ~8x fewer cycles per
// wave-step; same operations in the same order, hence the same bits).
template <typename T, int METHOD, int W, typename M = ProgModel<T, W>>
__global__ void __launch_bounds__(kBlock) trajectory_prog_kernel(const ProgArgs<T> p) {
  constexpr bool kNeedU = METHOD == kSrk;
  using V = Vec<T, W>;
  const int64_t lane = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t i = lane * W;
  if (i >= p.n) return;
  const int64_t col = i % p.d;
  const Pack<T, W> y_init = load<T, W>(p.y0, i);
  V y;
#pragma unroll
  for (int q = 0; q < W; ++q) y.v[q] = y_init.v[q];
  M m;
  m.setup(p, col);
  const NoiseKey key = launch_key(p.key, p.key_dev);
  const bool scalar_noise = p.scalar_noise != 0;
  const uint64_t elem = key.elem0 + (uint64_t)(scalar_noise ? i / p.d : i);
  int j = 0;
  int next_out = next_output_step<false>(p.out_step, 0, p.n_out);
  for (int k = 0; k < p.n_steps; ++k) {
    const StepRow<T> r = step_row<false>(p.rows + (int64_t)k * 8, p.cells, k);
    V w((T)0), u((T)0);
    draw_increment<T, W, kNeedU, /*PAIRS=*/false>(PlainStepNoise(key, r.cell), r, elem, scalar_noise, w.v, u.v);
    stage_times<T, METHOD>(r.t0(), r.dt, m.tslot);
    const V y1 = scheme_step<T, METHOD, V, M, V>(y, m, w, u, r.dt, r.half_dt, r.rdt, r.sqrt_dt);
    emit_outputs<false, W>(p, i, k, j, next_out, y.v, y1.v);
    y = y1;
  }
}

// ---- ... and their path-wise sensitivities ------------------------------------------------------------------------------
// Training THROUGH the solver (ordinary autograd through torchsde.sdeint, _core/sdeint.py:27-112) for an SDE stated as
// expression programs: the same programs run on forward-mode dual numbers. Tangent slot 0 is d/dy0; slots 1..4 belong to up
// to four constant rows (`param_slot[k]` = slot of row k, or -1): the per-channel parameters of the user's module. Every
// recursion is elementwise, so each tangent is one more scalar recursion in registers -- what `trajectory_kernel<.., SENS>`
// does for the affine form, for arbitrary elementwise code.
template <typename T>
TSDE_D Dual<T> operator-(const Dual<T>& x, const Dual<T>& y) {
  Dual<T> r;
  r.v = x.v - y.v;
#pragma unroll
  for (int i = 0; i < kSens; ++i) r.d[i] = x.d[i] - y.d[i];
  return r;
}
template <typename T>
TSDE_D Dual<T> operator*(const Dual<T>& x, const Dual<T>& y) {
  Dual<T> r;
  r.v = x.v * y.v;
#pragma unroll
  for (int i = 0; i < kSens; ++i) r.d[i] = x.d[i] * y.v + x.v * y.d[i];
  return r;
}
template <typename T>
TSDE_D Dual<T> operator/(const Dual<T>& x, const Dual<T>& y) {
  Dual<T> r;
  const T inv = (T)1 / y.v;
  r.v = x.v / y.v;
#pragma unroll
  for (int i = 0; i < kSens; ++i) r.d[i] = (x.d[i] - r.v * y.d[i]) * inv;
  return r;
}
// phi(x) with derivative `slope` at x.v
template <typename T>
TSDE_D Dual<T> chain(const Dual<T>& x, T value, T slope) {
  Dual<T> r;
  r.v = value;
#pragma unroll
  for (int i = 0; i < kSens; ++i) r.d[i] = slope * x.d[i];
  return r;
}

template <typename T>
struct ProgSensArgs;

template <typename T>
struct ProgSensModel {
  using S = Dual<T>;
  TSDE_D void setup(const ProgSensArgs<T>& q, int64_t column);
  const uint32_t* code;
  int f_len, g_len, dg_len;
  const T* consts;
  const int8_t* param_slot;        // per constant row: tangent slot 1..4, or -1 (kernel arguments, uniform)
  int64_t d, col;
  T tslot[4];

  TSDE_D S constant(uint32_t k) const {
    S c(consts[(int64_t)k * d + col]);
    const int slot = param_slot[k];
    if (slot > 0) c.d[slot] = (T)1;
    return c;
  }

  TSDE_D S run(const uint32_t* prog, int len, const S& x, const T time) const {
    S s0((T)0), s1((T)0), s2((T)0), s3((T)0);
    uint32_t fetched = prog[0];
    for (int pc = 0; pc < len; ++pc) {
      const uint32_t ins = fetched;
      fetched = prog[pc + 1 < len ? pc + 1 : pc];
      const uint32_t op = ins & 0xFFu, src = (ins >> 8) & 0xFFu, k = ins >> 16;
      if (op < kOpNeg) {
        S a = s0, b;
        if (src == kSrcStack) {
          b = s0;
          a = s1;
          s1 = s2;
          s2 = s3;
        } else if (src == kSrcConst) {
          b = constant(k);
        } else if (src == kSrcTime) {
          b = S(time);
        } else {
          b = x;
        }
        switch (op) {
          case kOpLoad:
            s3 = s2;
            s2 = s1;
            s1 = s0;
            s0 = b;
            break;
          case kOpAdd: s0 = a + b; break;
          case kOpSub: s0 = a - b; break;
          case kOpRsub: s0 = b - a; break;
          case kOpMul: s0 = a * b; break;
          case kOpDiv: s0 = a / b; break;
          default: s0 = b / a; break;
        }
      } else {
        const T v = s0.v;
        switch (op) {
          case kOpNeg: s0 = chain(s0, -v, (T)-1); break;
          case kOpExp: { const T e = exp(v); s0 = chain(s0, e, e); break; }
          case kOpLog: s0 = chain(s0, log(v), (T)1 / v); break;
          case kOpSin: s0 = chain(s0, sin(v), cos(v)); break;
          case kOpCos: s0 = chain(s0, cos(v), -sin(v)); break;
          case kOpTanh: { const T t = tanh(v); s0 = chain(s0, t, (T)1 - t * t); break; }
          case kOpSigmoid: { const T g = (T)1 / ((T)1 + exp(-v)); s0 = chain(s0, g, g * ((T)1 - g)); break; }
          case kOpSoftplus: {
            // slope z / (z + 1) with z = exp(v), as torch's softplus_backward forms it: for v > 0 the rounding of z cancels,
            // where 1 / (1 + exp(-v)) rounds 1 + exp(-v) at the spacing of 1 and so costs a whole ulp of a result below 1
            // (1.3 ulp against 0.5 in [4, 8), profiles/README.md); z is used for v <= 20 only, where it is finite
            const T z = exp(v);
            s0 = chain(s0, v > (T)20 ? v : log1p(z), v > (T)20 ? (T)1 : z / (z + (T)1));
            break;
          }
          case kOpSqrt: { const T r = sqrt(v); s0 = chain(s0, r, (T)0.5 / r); break; }
          case kOpAbs: s0 = chain(s0, fabs(v), v > (T)0 ? (T)1 : (v < (T)0 ? (T)-1 : (T)0)); break;
          case kOpRelu: s0 = chain(s0, v > (T)0 ? v : (T)0, v > (T)0 ? (T)1 : (T)0); break;
          case kOpRecip: { const T r = (T)1 / v; s0 = chain(s0, r, -(r * r)); break; }
          case kOpSquare: s0 = chain(s0, v * v, (T)2 * v); break;
          case kOpCube: s0 = chain(s0, (v * v) * v, (T)3 * (v * v)); break;
          default:
            s3 = s2;
            s2 = s1;
            s1 = s0;
            break;
        }
      }
    }
    return s0;
  }
  template <int SLOT>
  TSDE_D S f(const S& x) const { return run(code, f_len, x, tslot[SLOT]); }
  template <int SLOT>
  TSDE_D S g(const S& x) const { return run(code + f_len, g_len, x, tslot[SLOT]); }
  template <int SLOT>
  TSDE_D S gdg(const S& x, const S& gv, T v2) const { return (gv * v2) * run(code + f_len + g_len, dg_len, x, tslot[SLOT]); }
};

constexpr int kProgParamRows = 64;

template <typename T>
struct ProgSensArgs {
  ProgArgs<T> base;
  T* sens;                          // (n_out, kSens, n)
  int8_t param_slot[kProgParamRows];
};

template <typename T>
TSDE_D void ProgSensModel<T>::setup(const ProgSensArgs<T>& q, int64_t column) {
  code = q.base.code;
  f_len = q.base.f_len;
  g_len = q.base.g_len;
  dg_len = q.base.dg_len;
  consts = q.base.consts;
  param_slot = q.param_slot;
  d = q.base.d;
  col = column;
}

// One element per lane (the duals are six values wide); values AND sensitivities of every requested output.
// (`M`: the interpreter, or the same programs as generated straight-line code on dual numbers -- specialise.py.)
template <typename T, int METHOD, typename M = ProgSensModel<T>>
__global__ void __launch_bounds__(kBlock) trajectory_prog_sens_kernel(const ProgSensArgs<T> q) {
  constexpr bool kNeedU = METHOD == kSrk;
  const ProgArgs<T>& p = q.base;
  using S = Dual<T>;
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= p.n) return;
  M m;
  m.setup(q, i % p.d);
  S y(p.y0[i]);
  y.d[0] = (T)1;
  const NoiseKey key = launch_key(p.key, p.key_dev);
  const uint64_t elem = key.elem0 + (uint64_t)(p.scalar_noise ? i / p.d : i);
  int j = 0;
  int next_out = next_output_step<false>(p.out_step, 0, p.n_out);
  for (int k = 0; k < p.n_steps; ++k) {
    const StepRow<T> r = step_row<false>(p.rows + (int64_t)k * 8, p.cells, k);
    T w[1], u[1] = {(T)0};   // (scalar noise: `elem` is the row, and one element meets one increment either way)
    draw_increment<T, 1, kNeedU, /*PAIRS=*/false>(PlainStepNoise(key, r.cell), r, elem, false, w, u);
    stage_times<T, METHOD>(r.t0(), r.dt, m.tslot);
    const S y1 = scheme_step<T, METHOD, S, M>(y, m, w[0], u[0], r.dt, r.half_dt, r.rdt, r.sqrt_dt);
    if (__builtin_expect(k + 1 == next_out, 0)) {
      while (j < p.n_out && p.out_step[j] == k + 1) {
        const T w0 = p.out_w[2 * j], w1 = p.out_w[2 * j + 1];
        const bool exact = (w0 == (T)0 && w1 == (T)1);
        const S o = exact ? y1 : (w0 * y + w1 * y1);
        p.ys[(int64_t)j * p.n + i] = o.v;
#pragma unroll
        for (int s = 0; s < kSens; ++s) q.sens[((int64_t)j * kSens + s) * p.n + i] = o.d[s];
        ++j;
      }
      next_out = next_output_step<false>(p.out_step, j, p.n_out);
    }
    y = y1;
  }
}

// ---- row-coupled systems and their path-wise sensitivities ---------------------------------------------------------------
// Training THROUGH the solver for a small row-coupled system (torchsde_amd/recognise_rows.py: channels that read each other):
// one lane owns a whole row, as in `trajectory_prog_kernel` with W = D and a generated model, and beside its D values it
// carries NT tangent planes of D values -- d/dy0 of the row (D planes, when y0 needs a gradient), then one plane per trainable
// scalar constant of the user's module. The planes are not diagonal: channel c depends on channel c' of y0. A generated model
// (specialise.source_rows_sens) evaluates the system's statements on `Tan`, a scalar with NT tangents; the schemes run on
// `RowTan`, a row of them stored plane by plane, with the Brownian increment a plain Vec<T, D>.
template <typename T, int NT>
struct Tan {
  T v;
  T d[NT];
  Tan() = default;
  TSDE_D explicit Tan(T value) : v(value) {
#pragma unroll
    for (int i = 0; i < NT; ++i) d[i] = (T)0;
  }
};
// a constant whose own tangent slot K is 1: literal, so that the compiler folds the zeros of every other slot
template <int K, typename T, int NT>
TSDE_D Tan<T, NT> tan_seed(T value) {
  Tan<T, NT> r(value);
  r.d[K] = (T)1;
  return r;
}
#define TSDE_TAN_LINEAR(OP)                                                                    \
  template <typename T, int NT>                                                                \
  TSDE_D Tan<T, NT> operator OP(const Tan<T, NT>& x, const Tan<T, NT>& y) {                    \
    Tan<T, NT> r;                                                                              \
    r.v = x.v OP y.v;                                                                          \
    _Pragma("unroll") for (int i = 0; i < NT; ++i) r.d[i] = x.d[i] OP y.d[i];                  \
    return r;                                                                                  \
  }                                                                                            \
  template <typename T, int NT>                                                                \
  TSDE_D Tan<T, NT> operator OP(const Tan<T, NT>& x, T s) {                                    \
    Tan<T, NT> r = x;                                                                          \
    r.v = x.v OP s;                                                                            \
    return r;                                                                                  \
  }
TSDE_TAN_LINEAR(+)
TSDE_TAN_LINEAR(-)
#undef TSDE_TAN_LINEAR
template <typename T, int NT>
TSDE_D Tan<T, NT> operator+(T s, const Tan<T, NT>& x) {
  Tan<T, NT> r = x;
  r.v = s + x.v;
  return r;
}
template <typename T, int NT>
TSDE_D Tan<T, NT> operator-(T s, const Tan<T, NT>& x) {
  Tan<T, NT> r;
  r.v = s - x.v;
#pragma unroll
  for (int i = 0; i < NT; ++i) r.d[i] = -x.d[i];
  return r;
}
template <typename T, int NT>
TSDE_D Tan<T, NT> operator*(const Tan<T, NT>& x, const Tan<T, NT>& y) {
  Tan<T, NT> r;
  r.v = x.v * y.v;
#pragma unroll
  for (int i = 0; i < NT; ++i) r.d[i] = x.d[i] * y.v + x.v * y.d[i];
  return r;
}
template <typename T, int NT>
TSDE_D Tan<T, NT> operator*(const Tan<T, NT>& x, T s) {
  Tan<T, NT> r;
  r.v = x.v * s;
#pragma unroll
  for (int i = 0; i < NT; ++i) r.d[i] = x.d[i] * s;
  return r;
}
template <typename T, int NT>
TSDE_D Tan<T, NT> operator*(T s, const Tan<T, NT>& x) {
  Tan<T, NT> r;
  r.v = s * x.v;
#pragma unroll
  for (int i = 0; i < NT; ++i) r.d[i] = s * x.d[i];
  return r;
}
// (quotients as `Dual`'s: the tangent from the rounded quotient and one reciprocal)
template <typename T, int NT>
TSDE_D Tan<T, NT> operator/(const Tan<T, NT>& x, const Tan<T, NT>& y) {
  Tan<T, NT> r;
  const T inv = (T)1 / y.v;
  r.v = x.v / y.v;
#pragma unroll
  for (int i = 0; i < NT; ++i) r.d[i] = (x.d[i] - r.v * y.d[i]) * inv;
  return r;
}
template <typename T, int NT>
TSDE_D Tan<T, NT> operator/(const Tan<T, NT>& x, T s) {
  Tan<T, NT> r;
  const T inv = (T)1 / s;
  r.v = x.v / s;
#pragma unroll
  for (int i = 0; i < NT; ++i) r.d[i] = x.d[i] * inv;
  return r;
}
template <typename T, int NT>
TSDE_D Tan<T, NT> operator/(T s, const Tan<T, NT>& y) {
  Tan<T, NT> r;
  const T inv = (T)1 / y.v;
  r.v = s / y.v;
#pragma unroll
  for (int i = 0; i < NT; ++i) r.d[i] = -(r.v * y.d[i]) * inv;
  return r;
}
// phi(x) with derivative `slope` at x.v (the slope rules are those of the elementwise programs: specialise._DUAL_HELPERS)
template <typename T, int NT>
TSDE_D Tan<T, NT> chain(const Tan<T, NT>& x, T value, T slope) {
  Tan<T, NT> r;
  r.v = value;
#pragma unroll
  for (int i = 0; i < NT; ++i) r.d[i] = slope * x.d[i];
  return r;
}

// A row's D values and NT tangent planes; what `scheme_step`, `drift_diffusion_update` and the SRID2 helpers do to a state:
// sums of states, products with a step scalar (either side) and with the row's increments.
template <typename T, int D, int NT>
struct RowTan {
  Vec<T, D> v;
  Vec<T, D> t[NT];
  RowTan() = default;
  TSDE_D explicit RowTan(T s) : v(s) {
#pragma unroll
    for (int k = 0; k < NT; ++k) t[k] = Vec<T, D>((T)0);
  }
  // channel c as a scalar with its tangents, and back
  TSDE_D Tan<T, NT> channel(int c) const {
    Tan<T, NT> r;
    r.v = v.v[c];
#pragma unroll
    for (int k = 0; k < NT; ++k) r.d[k] = t[k].v[c];
    return r;
  }
  TSDE_D void set(int c, const Tan<T, NT>& x) {
    v.v[c] = x.v;
#pragma unroll
    for (int k = 0; k < NT; ++k) t[k].v[c] = x.d[k];
  }
  TSDE_D void set(int c, T x) {
    v.v[c] = x;
#pragma unroll
    for (int k = 0; k < NT; ++k) t[k].v[c] = (T)0;
  }
};
template <typename T, int D, int NT>
TSDE_D RowTan<T, D, NT> operator+(const RowTan<T, D, NT>& x, const RowTan<T, D, NT>& y) {
  RowTan<T, D, NT> r;
  r.v = x.v + y.v;
#pragma unroll
  for (int k = 0; k < NT; ++k) r.t[k] = x.t[k] + y.t[k];
  return r;
}
template <typename T, int D, int NT>
TSDE_D RowTan<T, D, NT> operator+(const RowTan<T, D, NT>& x, T s) {
  RowTan<T, D, NT> r = x;
  r.v = x.v + s;
  return r;
}
// `N`: a step scalar T, or the row's increments Vec<T, D>
template <typename T, int D, int NT, typename N>
TSDE_D RowTan<T, D, NT> operator*(const RowTan<T, D, NT>& x, const N& s) {
  RowTan<T, D, NT> r;
  r.v = x.v * s;
#pragma unroll
  for (int k = 0; k < NT; ++k) r.t[k] = x.t[k] * s;
  return r;
}
template <typename T, int D, int NT>
TSDE_D RowTan<T, D, NT> operator*(T s, const RowTan<T, D, NT>& x) {
  RowTan<T, D, NT> r;
  r.v = s * x.v;
#pragma unroll
  for (int k = 0; k < NT; ++k) r.t[k] = s * x.t[k];
  return r;
}

template <typename T>
struct RowsSensArgs {
  ProgArgs<T> base;         // consts: one scalar per constant (n_const of them); no programs, no scalar noise
  T* sens;                  // (n_out, NT, rows, d)
};

// One lane per row; values AND sensitivities of every requested output. `M`: the generated model on RowTan<T, D, NT>;
// `M::kStateSlots`: y0 carries the first D tangent slots. The increments, the step header and the stage times are those of
// `trajectory_prog_kernel` with W = D, and the value part of every operation is that kernel's: the same `ys`, bit for bit.
template <typename T, int METHOD, int D, int NT, typename M>
__global__ void __launch_bounds__(kBlock) trajectory_rows_sens_kernel(const RowsSensArgs<T> q) {
  constexpr bool kNeedU = METHOD == kSrk;
  using V = Vec<T, D>;
  using S = RowTan<T, D, NT>;
  const ProgArgs<T>& p = q.base;
  const int64_t lane = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t i = lane * D;
  if (i >= p.n) return;
  const Pack<T, D> y_init = load<T, D>(p.y0, i);
  S y((T)0);
#pragma unroll
  for (int c = 0; c < D; ++c) {
    y.v.v[c] = y_init.v[c];
    if constexpr (M::kStateSlots) y.t[c].v[c] = (T)1;
  }
  M m;
  m.setup(p, 0);
  const NoiseKey key = launch_key(p.key, p.key_dev);
  const uint64_t elem = key.elem0 + (uint64_t)i;
  int j = 0;
  int next_out = next_output_step<false>(p.out_step, 0, p.n_out);
  for (int k = 0; k < p.n_steps; ++k) {
    const StepRow<T> r = step_row<false>(p.rows + (int64_t)k * 8, p.cells, k);
    V w((T)0), u((T)0);
    draw_increment<T, D, kNeedU, /*PAIRS=*/false>(PlainStepNoise(key, r.cell), r, elem, false, w.v, u.v);
    stage_times<T, METHOD>(r.t0(), r.dt, m.tslot);
    const S y1 = scheme_step<T, METHOD, S, M, V>(y, m, w, u, r.dt, r.half_dt, r.rdt, r.sqrt_dt);
    if (__builtin_expect(k + 1 == next_out, 0)) {
      while (j < p.n_out && p.out_step[j] == k + 1) {
        const T w0 = p.out_w[2 * j], w1 = p.out_w[2 * j + 1];
        const bool exact = (w0 == (T)0 && w1 == (T)1);
        Pack<T, D> ov;
#pragma unroll
        for (int c = 0; c < D; ++c) ov.v[c] = exact ? y1.v.v[c] : (w0 * y.v.v[c] + w1 * y1.v.v[c]);
        store<T, D>(p.ys + (int64_t)j * p.n, i, ov);
#pragma unroll
        for (int s = 0; s < NT; ++s) {
#pragma unroll
          for (int c = 0; c < D; ++c) ov.v[c] = exact ? y1.t[s].v[c] : (w0 * y.t[s].v[c] + w1 * y1.t[s].v[c]);
          store<T, D>(q.sens + ((int64_t)j * NT + s) * p.n, i, ov);
        }
        ++j;
      }
      next_out = next_output_step<false>(p.out_step, j, p.n_out);
    }
    y = y1;
  }
}

// ---- row-coupled systems with a diffusion MATRIX: general, scalar and additive noise -----------------------------------
// One lane per row, as `trajectory_prog_kernel` with W = D, but the row meets MN Brownian channels and its diffusion is a
// (D, MN) matrix: y1 = (y0 + cf*f) + cg * sum_k g[i][k] dW[k], the stepwise route's order (steps.hip, the general-noise
// contraction). The matrix never exists as an array: the generated model (specialise.source_rows_general) holds this step's
// increments, `m.w`, and its `g<SLOT>(y)` IS the contraction -- per row i the sum over k in increasing k, straight-line, no
// term for an entry that is structurally zero -- so that the schemes run through `scheme_step` with the unit as their noise
// operand (g * 1 is g, bit for bit). The field is (rows, MN): row r meets elements r * MN .. r * MN + MN - 1 (scalar noise:
// MN = 1, element r). Euler, midpoint, Heun, Euler-Heun: the schemes the reference has for general noise.
// The argument block is `ProgArgs` as it is (consts: one scalar per constant; no programs, no scalar-noise flag): the number
// of Brownian channels is the template argument MN, checked against the solve's m on the host (`launch_rows_general`).
template <typename T, int METHOD, int D, int MN, typename M>
__global__ void __launch_bounds__(kBlock) trajectory_rows_general_kernel(const ProgArgs<T> p) {
  static_assert(METHOD == kEuler || METHOD == kMidpoint || METHOD == kHeun || METHOD == kEulerHeun,
                "general noise: Euler, midpoint, Heun, Euler-Heun");
  using V = Vec<T, D>;
  const int64_t row = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t i = row * D;
  if (i >= p.n) return;
  const Pack<T, D> y_init = load<T, D>(p.y0, i);
  V y;
#pragma unroll
  for (int c = 0; c < D; ++c) y.v[c] = y_init.v[c];
  M m;
  m.setup(p, 0);
  const NoiseKey key = launch_key(p.key, p.key_dev);
  const uint64_t elem = key.elem0 + (uint64_t)row * (uint64_t)MN;
  int j = 0;
  int next_out = next_output_step<false>(p.out_step, 0, p.n_out);
  for (int k = 0; k < p.n_steps; ++k) {
    const StepRow<T> r = step_row<false>(p.rows + (int64_t)k * 8, p.cells, k);
    T unused[MN];
    // (MN = 4: the row's increments are ONE Philox quad -- `launch_rows_general` takes only shards that start on a quad)
    draw_increment<T, MN, /*NEED_U=*/false, /*PAIRS=*/false>(PlainStepNoise(key, r.cell), r, elem, false, m.w, unused);
    stage_times<T, METHOD>(r.t0(), r.dt, m.tslot);
    const V y1 = scheme_step<T, METHOD, V, M, T>(y, m, (T)1, (T)0, r.dt, r.half_dt, r.rdt, r.sqrt_dt);
    emit_outputs<false, D>(p, i, k, j, next_out, y.v, y1.v);
    y = y1;
  }
}

// ---- additive noise: the drift as a program, the diffusion as a table ---------------------------------------------------
// Noise type "additive" (base_sde.py:101-102; the reference's ExAdditive, tests/problems.py:106-132): g depends on t only
// and every batch row meets the same (d, m) matrix. The host evaluates the user's g at every stage time of the solve
// (recognise.RecognisedAdditive: one batched call) and hands the kernel `gtab[step][slot][j][c]` = g(t)[c, j]; a matrix that
// does not depend on t is one slot with stride 0. A lane holds W channels of its row, draws the row's m increments itself
// (the field is (rows, m): element row * m + j -- a lane of the same row draws the same numbers) and contracts them with its
// W rows of G in ascending j. Schemes: Euler (euler.py:29-37; Milstein with additive noise is the same step, milstein.py:
// base_sde.py:157-158 gdg = 0), midpoint (midpoint.py:29-45), SRK = SRA1 (srk.py:90-111, tableaus/sra1.py) with the
// operation order of the stepwise route's `tsde_step_general_w` calls (solvers.SRK._advance_additive).
template <typename T>
struct ProgAdditiveArgs {
  ProgArgs<T> base;         // g_len = dg_len = 0
  const T* gtab;
  int64_t step_stride;      // elements between the tables of consecutive steps (0: the matrix does not depend on t)
  int64_t slot_stride;      // elements between the stage-time slots of one step (m * d)
  int32_t m;                // Brownian channels per row, <= MP of the instantiation
  int32_t quads;            // != 0: m % 4 == 0 and elem0 % 4 == 0, a row's channels are whole Philox quads
};

template <typename T, int METHOD, int W, int MP, typename M = ProgModel<T, W>>
__global__ void __launch_bounds__(kBlock) trajectory_prog_additive_kernel(const ProgAdditiveArgs<T> q) {
  constexpr bool kNeedU = METHOD == kSrk;
  using V = Vec<T, W>;
  const ProgArgs<T>& p = q.base;
  const int64_t lane = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t i = lane * W;
  if (i >= p.n) return;
  const int64_t col = i % p.d;
  const Pack<T, W> y_init = load<T, W>(p.y0, i);
  V y;
#pragma unroll
  for (int e = 0; e < W; ++e) y.v[e] = y_init.v[e];
  M m;                      // (the interpreter, or the drift program as generated code: specialise.py)
  m.setup(p, col);
  const NoiseKey key = launch_key(p.key, p.key_dev);
  const int nm = q.m;
  const uint64_t elem = key.elem0 + (uint64_t)(i / p.d) * (uint64_t)nm;      // the row's first Brownian channel
  int j = 0;
  int next_out = next_output_step<false>(p.out_step, 0, p.n_out);
  for (int k = 0; k < p.n_steps; ++k) {
    const T* row = p.rows + (int64_t)k * 8;   // wave-uniform
    const T dt = row[0], half_dt = row[1], rdt = row[2], sw = row[4], sh = row[5], th = row[6], t0 = row[7];
    const uint32_t cell = p.cells[k];
    T wv[MP], uv[MP];
#pragma unroll
    for (int c = 0; c < MP; ++c) wv[c] = uv[c] = (T)0;
    if (q.quads) {
#pragma unroll
      for (int c = 0; c < MP / 4; ++c) {
        if (4 * c < nm) {
          T z[4];
          if constexpr (kNeedU) normal4_pairs<T>(key, (elem >> 2) + (uint64_t)c, cell, 0, kStreamW, z);   // (SRK: as above)
          else normal4<T>(key, (elem >> 2) + (uint64_t)c, cell, 0, kStreamW, z);
#pragma unroll
          for (int e = 0; e < 4; ++e) wv[4 * c + e] = z[e] * sw;
          if constexpr (kNeedU) {
            normal4_pairs<T>(key, (elem >> 2) + (uint64_t)c, cell, 0, kStreamH, z);
#pragma unroll
            for (int e = 0; e < 4; ++e) uv[4 * c + e] = th * ((T)0.5 * wv[4 * c + e] + z[e] * sh);
          }
        }
      }
    } else {
#pragma unroll
      for (int c = 0; c < MP; ++c) {
        if (c < nm) {
          wv[c] = normal1<T>(key, elem + (uint64_t)c, cell, 0, kStreamW) * sw;
          if constexpr (kNeedU) uv[c] = th * ((T)0.5 * wv[c] + normal1<T>(key, elem + (uint64_t)c, cell, 0, kStreamH) * sh);
        }
      }
    }
    const T* gk = q.gtab + (int64_t)k * q.step_stride + col;
    // sum_j G[c, j] * weight(j) for this lane's channels, ascending j
    auto contract = [&](const T* G, auto weight) {
      V acc((T)0);
#pragma unroll
      for (int c = 0; c < MP; ++c) {
        if (c < nm) {
          const Pack<T, W> gp = load<T, W>(G, (int64_t)c * p.d);
          const T wc = weight(c);
#pragma unroll
          for (int e = 0; e < W; ++e) acc.v[e] = c == 0 ? gp.v[e] * wc : acc.v[e] + gp.v[e] * wc;
        }
      }
      return acc;
    };
    m.tslot[0] = t0;
    V y1;
    if constexpr (METHOD == kEuler) {
      y1 = (y + m.template f<0>(y) * dt) + contract(gk, [&](int c) { return wv[c]; });
    } else if constexpr (METHOD == kMidpoint) {
      m.tslot[1] = t0 + (T)0.5 * dt;
      const V yp = (y + m.template f<0>(y) * half_dt) + (T)0.5 * contract(gk, [&](int c) { return wv[c]; });
      y1 = (y + m.template f<1>(yp) * dt) + contract(gk + q.slot_stride, [&](int c) { return wv[c]; });
    } else {
      // slot 0: g(t0 + C1[0] dt) = g(t0 + dt); slot 1: g(t0 + C1[1] dt) = g(t0)
      m.tslot[1] = t0 + (T)0.75 * dt;
      const V f0 = m.template f<0>(y);
      const V h = (y + ((T)0.75 * f0) * dt) + contract(gk, [&](int c) { return ((T)1.5 * uv[c]) * rdt; });
      const V acc = (y + ((T)(1.0 / 3) * f0) * dt) + contract(gk, [&](int c) { return ((T)1 * wv[c]) + ((T)-1 * uv[c]) * rdt; });
      const V f1 = m.template f<1>(h);
      y1 = (acc + ((T)(2.0 / 3) * f1) * dt) +
           contract(gk + q.slot_stride, [&](int c) { return ((T)0 * wv[c]) + ((T)1 * uv[c]) * rdt; });
    }
    if (__builtin_expect(k + 1 == next_out, 0)) {
      while (j < p.n_out && p.out_step[j] == k + 1) {
        const T w0 = p.out_w[2 * j], w1 = p.out_w[2 * j + 1];
        const bool exact = (w0 == (T)0 && w1 == (T)1);
        Pack<T, W> ov;
#pragma unroll
        for (int e = 0; e < W; ++e) ov.v[e] = exact ? y1.v[e] : (w0 * y.v[e] + w1 * y1.v[e]);
        store<T, W>(p.ys + (int64_t)j * p.n, i, ov);
        ++j;
      }
      next_out = next_output_step<false>(p.out_step, j, p.n_out);
    }
    y = y1;
  }
}

// ---- launching a program kernel ---------------------------------------------------------------------------------------------
// Written once, for the interpreter (`launch_trajectory_prog_diag`, `launch_trajectory_prog_additive` below) and for the units
// torchsde_amd/specialise.py generates: such a unit is a model struct plus one call of these helpers with that model. They are
// templates, so a unit instantiates the kernels of its own model and nothing else.
inline NoiseKey noise_key(uint64_t entropy, uint64_t elem0) {
  NoiseKey k;
  k.k0 = (uint32_t)entropy;
  k.k1 = (uint32_t)(entropy >> 32);
  k.elem0 = elem0;
  return k;
}

// `code`: the interpreter's words, the f, g and dg programs back to back (at most kProgWords: the caller checks); a generated
// model has its programs in its code and passes none.
template <typename T>
static ProgArgs<T> prog_args(void* ys, const void* y0, int64_t rows, int64_t d, const void* consts, int n_const,
                             int scalar_noise, const tsde_traj_t* tr, NoiseKey key, const uint64_t* key_dev,
                             const uint32_t* code = nullptr, int f_len = 0, int g_len = 0, int dg_len = 0) {
  ProgArgs<T> p;
  traj_common<T>(p, ys, y0, rows, d, tr, key, key_dev);
  p.consts = (const T*)consts;
  p.f_len = f_len;
  p.g_len = g_len;
  p.dg_len = dg_len;
  p.n_const = n_const;
  p.scalar_noise = scalar_noise;
  for (int w = 0; w < kProgWords; ++w) p.code[w] = (code && w < f_len + g_len + dg_len) ? code[w] : 0u;
  return p;
}

template <typename T>
static ProgSensArgs<T> prog_sens_args(const ProgArgs<T>& base, void* sens, const int8_t* param_slot) {
  ProgSensArgs<T> q;
  q.base = base;
  q.sens = (T*)sens;
  for (int k = 0; k < kProgParamRows; ++k) q.param_slot[k] = (param_slot && k < base.n_const) ? param_slot[k] : (int8_t)-1;
  return q;
}

// `base`: g_len = dg_len = 0 and no scalar noise; `gtab`: (m, d), or one such matrix per stage time of every step
template <typename T>
static ProgAdditiveArgs<T> prog_additive_args(const ProgArgs<T>& base, int64_t m, const void* gtab, int time_dependent,
                                              int method) {
  const int slots = method == kEuler ? 1 : 2;
  ProgAdditiveArgs<T> q;
  q.base = base;
  q.gtab = (const T*)gtab;
  q.slot_stride = time_dependent ? m * base.d : 0;
  q.step_stride = time_dependent ? (int64_t)slots * m * base.d : 0;
  q.m = (int32_t)m;
  q.quads = (m % 4 == 0 && base.key.elem0 % 4 == 0) ? 1 : 0;
  return q;
}

// One lane per W elements (W = d: per row, the row-coupled systems of specialise.source_rows). An empty problem launches nothing.
template <typename T, int METHOD, int W, typename M = ProgModel<T, W>>
static hipError_t launch_prog_w(const ProgArgs<T>& p, hipStream_t s) {
  if (nothing_to_do(p)) return hipSuccess;
  return launch_lanes(trajectory_prog_kernel<T, METHOD, W, M>, p.n / W, s, p);
}

// ... and with NT tangent planes per row (specialise.source_rows_sens); `sens`: (n_out, NT, rows, D)
template <typename T, int METHOD, int D, int NT, typename M>
static hipError_t launch_rows_sens(const ProgArgs<T>& p, void* sens, hipStream_t s) {
  if (nothing_to_do(p)) return hipSuccess;
  RowsSensArgs<T> q;
  q.base = p;
  q.sens = (T*)sens;
  return launch_lanes(trajectory_rows_sens_kernel<T, METHOD, D, NT, M>, p.n / D, s, q);
}

// ... and with a (D, MN) diffusion matrix (specialise.source_rows_general): one lane per row, `m` must be the unit's MN
template <typename T, int METHOD, int D, int MN, typename M>
static hipError_t launch_rows_general(const ProgArgs<T>& p, int64_t m, hipStream_t s) {
  if (m != MN || p.d != D) return hipErrorInvalidValue;
  // MN = 4: `draw_increment` reads a row's increments as one Philox quad. The field of a (rows, 4) Brownian motion starts
  // at element row_offset * 4, always on a quad; any other start is refused rather than drawn from the wrong elements
  if (MN == 4 && p.key.elem0 % 4 != 0) return hipErrorInvalidValue;
  if (nothing_to_do(p)) return hipSuccess;
  return launch_lanes(trajectory_rows_general_kernel<T, METHOD, D, MN, M>, p.n / D, s, p);
}

template <typename T, int METHOD, template <typename, int> class M = ProgModel>
static hipError_t launch_prog_m(const ProgArgs<T>& p, hipStream_t s) {
  const bool vec = may_vec(p) &&
                   (p.scalar_noise || p.key.elem0 % 4 == 0);   // scalar noise addresses the field by row: any elem0
  return vec ? launch_prog_w<T, METHOD, 4, M<T, 4>>(p, s) : launch_prog_w<T, METHOD, 1, M<T, 1>>(p, s);
}

template <typename T, int METHOD, typename M = ProgSensModel<T>>
static hipError_t launch_prog_sens_m(const ProgSensArgs<T>& q, hipStream_t s) {
  if (nothing_to_do(q.base)) return hipSuccess;
  return launch_lanes(trajectory_prog_sens_kernel<T, METHOD, M>, q.base.n, s, q);
}

// `MP`: the channel-count class (4, 8, 16), q.m <= MP
template <typename T, int METHOD, int MP, template <typename, int> class M = ProgModel>
static hipError_t launch_additive_mp(const ProgAdditiveArgs<T>& q, hipStream_t s) {
  const ProgArgs<T>& p = q.base;
  if (nothing_to_do(p)) return hipSuccess;
  const bool vec = may_vec(p, q.gtab);   // (the field is addressed by row and channel: no condition on elem0)
  if (vec) return launch_lanes(trajectory_prog_additive_kernel<T, METHOD, 4, MP, M<T, 4>>, p.n >> 2, s, q);
  return launch_lanes(trajectory_prog_additive_kernel<T, METHOD, 1, MP, M<T, 1>>, p.n, s, q);
}

template <typename T, int METHOD>
static hipError_t launch_additive_m(const ProgAdditiveArgs<T>& q, hipStream_t s) {
  if (q.m <= 4) return launch_additive_mp<T, METHOD, 4>(q, s);
  if (q.m <= 8) return launch_additive_mp<T, METHOD, 8>(q, s);
  if (q.m <= 16) return launch_additive_mp<T, METHOD, 16>(q, s);
  return hipErrorInvalidValue;
}

#ifndef TSDE_SPECIALISE_TU
hipError_t launch_trajectory_prog_additive(int dtype, void* ys, const void* y0, int64_t rows, int64_t d, int64_t m,
                                           const uint32_t* code, int f_len, const void* consts, int n_const, const void* gtab,
                                           int time_dependent, int method, const tsde_traj_t* tr, NoiseKey key,
                                           const uint64_t* key_dev, hipStream_t s) {
  if (f_len > kProgWords) return hipErrorInvalidValue;
  return by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    const ProgAdditiveArgs<T> q = prog_additive_args(
        prog_args<T>(ys, y0, rows, d, consts, n_const, 0, tr, key, key_dev, code, f_len), m, gtab, time_dependent, method);
    // Euler, midpoint and SRK only (the kernel has no other scheme, and none is instantiated)
    return dispatch_method(method, [&](auto m) {
      constexpr int METHOD = decltype(m)::value;
      if constexpr (METHOD == kEuler || METHOD == kMidpoint || METHOD == kSrk) return launch_additive_m<T, METHOD>(q, s);
      else return hipErrorInvalidValue;
    });
  });
}
#endif

// values, or (with `sens`) values and path-wise sensitivities
template <typename T, int METHOD>
static hipError_t launch_prog_diag_m(const ProgArgs<T>& p, void* sens, const int8_t* param_slot, hipStream_t s) {
  if (sens != nullptr) return launch_prog_sens_m<T, METHOD>(prog_sens_args(p, sens, param_slot), s);
  return launch_prog_m<T, METHOD>(p, s);
}

#ifndef TSDE_SPECIALISE_TU
hipError_t launch_trajectory_prog_diag(int dtype, void* ys, void* sens, const int8_t* param_slot, const void* y0, int64_t rows,
                                       int64_t d, const uint32_t* code, int f_len, int g_len, int dg_len, const void* consts,
                                       int n_const, int scalar_noise, int method, const tsde_traj_t* tr, NoiseKey key,
                                       const uint64_t* key_dev, hipStream_t s) {
  if (f_len + g_len + dg_len > kProgWords) return hipErrorInvalidValue;
  return by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    const ProgArgs<T> p =
        prog_args<T>(ys, y0, rows, d, consts, n_const, scalar_noise, tr, key, key_dev, code, f_len, g_len, dg_len);
    return dispatch_method(method, [&](auto m) { return launch_prog_diag_m<T, decltype(m)::value>(p, sens, param_slot, s); });
  });
}
#endif

}  // namespace tsde
