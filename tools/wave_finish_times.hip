// Diagnostic build of the affine trajectory kernel: when every wave of ONE launch started and ended, and on which SIMD.
// The kernels come from csrc/trajectory.hip, included as the specialised units include it, with TSDE_WAVE_STAMPS defined:
// each wave then stores two readings of the 100 MHz clock and its HW_ID / XCC_ID registers into a buffer of its own
// (`WaveStamp`); the shipped library is built without the macro. Build and run: tools/wave_finish_times.py.
//
//   wave_finish_times <rows> <d> <n_steps> <method: 0 Euler, 3 midpoint, ...> <flags: tsde_traj_t.flags> <out.bin>
//
// One warm-up launch and one stamped launch of the linear form (f = mu y, g = sigma y; dt = 2^-10, one output at the end),
// the headline workload's arguments. Writes (waves, 4) uint64: start, end, HW_ID | XCC_ID << 32, 0.
#define TSDE_SPECIALISE_TU 1
#define TSDE_WAVE_STAMPS 1
#include "../torchsde_amd/csrc/trajectory.hip"

#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(x)                                                                          \
  do {                                                                                 \
    hipError_t e_ = (x);                                                               \
    if (e_ != hipSuccess) {                                                            \
      printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__);            \
      return 1;                                                                        \
    }                                                                                  \
  } while (0)

template <typename X>
static hipError_t upload(const std::vector<X>& host, X** dev) {
  hipError_t e = hipMalloc((void**)dev, host.size() * sizeof(X));
  if (e != hipSuccess) return e;
  return hipMemcpy(*dev, host.data(), host.size() * sizeof(X), hipMemcpyHostToDevice);
}

int main(int argc, char** argv) {
  using namespace tsde;
  if (argc != 7) {
    printf("usage: %s rows d n_steps method flags out.bin\n", argv[0]);
    return 2;
  }
  const int64_t rows = atoll(argv[1]), d = atoll(argv[2]);
  const int n_steps = atoi(argv[3]), method = atoi(argv[4]);
  const uint32_t flags = (uint32_t)strtoul(argv[5], nullptr, 0);
  const int64_t n = rows * d;
  if (rows <= 0 || d <= 0 || d % 4 != 0 || n_steps <= 0 || (n >> 2) < kTrajVecMinGroups) {
    printf("needs d %% 4 == 0 and at least %lld 16-byte groups (the W = 4 form)\n", (long long)kTrajVecMinGroups);
    return 2;
  }
  const float dt = 1.0f / 1024.0f;
  std::vector<float> step_rows((size_t)n_steps * 8), y0((size_t)n, 0.1f), mu((size_t)d), sigma((size_t)d);
  std::vector<uint32_t> cells((size_t)n_steps);
  for (int k = 0; k < n_steps; ++k) {
    const float row[8] = {dt, 0.5f * dt, 1.0f / dt, 0.03125f, 0.03125f, sqrtf(dt / 12.0f), dt, k * dt};
    for (int c = 0; c < 8; ++c) step_rows[(size_t)k * 8 + c] = row[c];
    cells[k] = (uint32_t)k;
  }
  for (int64_t c = 0; c < d; ++c) {
    mu[c] = 0.05f + 0.001f * (float)c;
    sigma[c] = 0.2f + 0.001f * (float)c;
  }
  const std::vector<int32_t> out_step = {n_steps};
  const std::vector<float> out_w = {0.0f, 1.0f};
  const int64_t waves = ((n >> 2) + 63) / 64;

  float *d_rows, *d_y0, *d_mu, *d_sigma, *d_out_w, *d_ys;
  uint32_t* d_cells;
  int32_t* d_out_step;
  uint64_t* d_stamps;
  CK(upload(step_rows, &d_rows));
  CK(upload(y0, &d_y0));
  CK(upload(mu, &d_mu));
  CK(upload(sigma, &d_sigma));
  CK(upload(out_w, &d_out_w));
  CK(upload(cells, &d_cells));
  CK(upload(out_step, &d_out_step));
  CK(hipMalloc((void**)&d_ys, (size_t)n * sizeof(float)));
  CK(hipMalloc((void**)&d_stamps, (size_t)waves * 4 * sizeof(uint64_t)));
  CK(hipMemset(d_stamps, 0, (size_t)waves * 4 * sizeof(uint64_t)));

  tsde_traj_t tr = {};
  tr.step_rows = d_rows;
  tr.cells = d_cells;
  tr.out_step = d_out_step;
  tr.out_w = d_out_w;
  tr.n_steps = n_steps;
  tr.n_out = 1;
  tr.flags = flags;
  TrajArgs<float> p;
  traj_common<float>(p, d_ys, d_y0, rows, d, &tr, NoiseKey{20240601u, 0u, 0}, nullptr);
  p.sens = nullptr;
  p.a = d_mu;
  p.c = d_sigma;
  p.b = p.e = nullptr;
  p.cstride = 0;
  p.stamps = d_stamps;
  p.flags = tr.flags;
  const bool pow2 = (flags & TSDE_TRAJ_POW2_STEPS) != 0;
  for (int launch = 0; launch < 2; ++launch) {   // (the second launch's stamps overwrite the warm-up's)
    CK(dispatch_method(method, [&](auto m) { return launch_traj_m<float, decltype(m)::value>(p, true, pow2, 0); }));
    CK(hipDeviceSynchronize());
  }
  std::vector<uint64_t> stamps((size_t)waves * 4);
  CK(hipMemcpy(stamps.data(), d_stamps, stamps.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
  FILE* f = fopen(argv[6], "wb");
  if (!f || fwrite(stamps.data(), sizeof(uint64_t), stamps.size(), f) != stamps.size()) {
    printf("cannot write %s\n", argv[6]);
    return 1;
  }
  fclose(f);
  printf("%lld waves stamped -> %s\n", (long long)waves, argv[6]);
  return 0;
}
