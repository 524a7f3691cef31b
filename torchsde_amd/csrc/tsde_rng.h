// Counter-based Brownian noise source for the MI355X-native torchsde hot path.
//
// Replaces the reference's per-tree-node `torch.Generator(seed) + torch.randn(size)`
// (torchsde/_brownian/brownian_interval.py:30-32, seeds from numpy SeedSequence :336-339)
// with a stateless Philox-4x32-10 field: every normal is a pure function of
//   (entropy, global element index, cell index, in-cell tree node, stream)
// so any increment can be (re)generated in registers, in any order, on any shard.
//
// This header is shared by the device kernels and by the host-side helpers the C-ABI
// exports for known-answer tests (include/torchsde_amd.h: tsde_philox4x32_10).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define TSDE_HD __host__ __device__ __forceinline__
#define TSDE_D __device__ __forceinline__
#else
#define TSDE_HD inline
#endif

namespace tsde {

struct u32x4 {
  uint32_t x, y, z, w;
};

// a ^ b ^ c in one instruction on the device (gfx950 v_bitop3_b32, truth table 0x96); hipcc does not fuse the
// two xors of a Philox round on its own, and they are a third of the round's VALU work.
#if defined(__HIP_DEVICE_COMPILE__)
#define TSDE_XOR3(a, b, c) ((uint32_t)__builtin_amdgcn_bitop3_b32((a), (b), (c), 0x96))
#else
#define TSDE_XOR3(a, b, c) ((a) ^ (b) ^ (c))
#endif

// Philox-4x32-10 (Salmon et al., SC'11). One call = 4 x 32 random bits.
TSDE_HD u32x4 philox4x32_10(u32x4 c, uint32_t k0, uint32_t k1) {
  constexpr uint32_t kM0 = 0xD2511F53u, kM1 = 0xCD9E8D57u;
  constexpr uint32_t kW0 = 0x9E3779B9u, kW1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)kM0 * c.x;
    const uint64_t p1 = (uint64_t)kM1 * c.z;
    const u32x4 n = {TSDE_XOR3((uint32_t)(p1 >> 32), c.y, k0), (uint32_t)p1,
                     TSDE_XOR3((uint32_t)(p0 >> 32), c.w, k1), (uint32_t)p0};
    c = n;
    k0 += kW0;
    k1 += kW1;
  }
  return c;
}

// The same ten rounds with the two values of rounds 0 and 1 that depend on (c.y, c.z, k0) alone handed in. A solver's step
// loop draws node 0 of one cell per step: c.y, c.z and the key are the same for every lane, so `philox_head` is work for
// the scalar unit (plain ^ and *: TSDE_XOR3 is a vector-only instruction and would pull its operands into vector registers),
// and only what depends on the lane's own counter words c.x, c.w is left to the vector unit. Same words as
// philox4x32_10(c, k0, k1) for every input when `h` = philox_head(c.y, c.z, k0).
struct PhiloxHead {
  uint32_t x1;   // word x after round 0: hi(kM1 * c.z) ^ c.y ^ k0
  uint64_t px;   // round 1's product kM0 * x1
};

TSDE_HD PhiloxHead philox_head(uint32_t cy, uint32_t cz, uint32_t k0) {
  PhiloxHead h;
  h.x1 = (uint32_t)(((uint64_t)0xCD9E8D57u * cz) >> 32) ^ cy ^ k0;
  h.px = (uint64_t)0xD2511F53u * h.x1;
  return h;
}

TSDE_HD u32x4 philox4x32_10_headed(u32x4 c, uint32_t k0, uint32_t k1, const PhiloxHead& h) {
  constexpr uint32_t kM0 = 0xD2511F53u, kM1 = 0xCD9E8D57u;
  constexpr uint32_t kW0 = 0x9E3779B9u, kW1 = 0xBB67AE85u;
  {   // round 0: word x is h.x1
    const uint64_t p0 = (uint64_t)kM0 * c.x;
    const u32x4 n = {h.x1, kM1 * c.z, TSDE_XOR3((uint32_t)(p0 >> 32), c.w, k1), (uint32_t)p0};
    c = n;
    k0 += kW0;
    k1 += kW1;
  }
  {   // round 1: the product of word x is h.px; its high half meets the key before it meets the lane's word
    const uint64_t p1 = (uint64_t)kM1 * c.z;
    const u32x4 n = {TSDE_XOR3((uint32_t)(p1 >> 32), c.y, k0), (uint32_t)p1, c.w ^ ((uint32_t)(h.px >> 32) ^ k1),
                     (uint32_t)h.px};
    c = n;
    k0 += kW0;
    k1 += kW1;
  }
#pragma unroll
  for (int r = 2; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)kM0 * c.x;
    const uint64_t p1 = (uint64_t)kM1 * c.z;
    const u32x4 n = {TSDE_XOR3((uint32_t)(p1 >> 32), c.y, k0), (uint32_t)p1,
                     TSDE_XOR3((uint32_t)(p0 >> 32), c.w, k1), (uint32_t)p0};
    c = n;
    k0 += kW0;
    k1 += kW1;
  }
  return c;
}

// Noise streams of one tree node.
enum : uint32_t { kStreamW = 0, kStreamH = 1, kStreamA = 2 };

// Identity of the noise field a kernel draws from.
struct NoiseKey {
  uint32_t k0, k1;   // entropy (low / high 32 bits)
  uint64_t elem0;    // global index of this shard's element 0 in the (B_global * m) noise tensor
};

#if defined(__HIPCC__)
// The key a kernel draws with: entropy that lives in device memory (a captured graph replayed with fresh entropy)
// replaces the entropy the launch was given.
TSDE_D NoiseKey launch_key(NoiseKey key, const uint64_t* key_dev) {
  if (key_dev != nullptr) {
    const uint64_t ent = *key_dev;
    key.k0 = (uint32_t)ent;
    key.k1 = (uint32_t)(ent >> 32);
  }
  return key;
}
#endif

// Counter layout:
//   c0 = quad[31:0]            quad = global element index >> 2 (4 normals per Philox call)
//   c1 = cell                  top-level cell of the Brownian grid
//   c2 = node[31:0]            heap index of the in-cell bridge-tree node (0 = the cell's own draw)
//   c3 = stream<<30 | quad[51:32]<<10 | node[41:32]
TSDE_HD u32x4 noise_counter(uint64_t quad, uint32_t cell, uint64_t node, uint32_t stream) {
  u32x4 c;
  c.x = (uint32_t)quad;
  c.y = cell;
  c.z = (uint32_t)node;
  c.w = (stream << 30) | (((uint32_t)(quad >> 32) & 0xFFFFFu) << 10) | ((uint32_t)(node >> 32) & 0x3FFu);
  return c;
}

TSDE_HD u32x4 noise_bits(const NoiseKey& key, uint64_t quad, uint32_t cell, uint64_t node, uint32_t stream) {
  return philox4x32_10(noise_counter(quad, cell, node, stream), key.k0, key.k1);
}

#if defined(__HIPCC__)
// ---- Box-Muller on the device ------------------------------------------------------------------
// Canonical definition (what the CPU oracle evaluates in double precision):
//   u1 = (a + 0.5) / 2^32 in (0,1),  theta = 2*pi * b / 2^32,
//   n0 = sqrt(-2 ln u1) cos(theta),  n1 = sqrt(-2 ln u1) sin(theta).
// fp32: v_log_f32 / v_sqrt_f32 / v_sin_f32 / v_cos_f32 (the latter two take revolutions, so theta
// needs no range reduction). Near u1 -> 1 the log is replaced by the series of -ln(1-w), w = 1-u1
// computed exactly from ~a, so small radii keep full relative accuracy.

// First words at and above this take the series: u1 >= 15/16, one pair in 16.
constexpr uint32_t kSeriesFrom = 0xF0000000u;

// The small-radius value of -2 ln u1 as a function of the pair's first word.
TSDE_D float box_muller_series(uint32_t a) {
  const float w = fmaf((float)(~a), 0x1p-32f, 0x1p-33f);
  // Horner of 2 * (1 + w/2 + w^2/3 + w^3/4 + w^4/5 + w^5/6) with the 2 folded into the coefficients. Doubling a float is
  // exact (nothing here is near overflow or subnormal), so each coefficient is exactly twice the plain one, doubling
  // commutes with the single rounding of every fmaf, and p is bit for bit twice the plain polynomial; w * p then rounds
  // to the same float as (2 * w) * (p / 2) did (tests/test_box_muller_series.py) -- one instruction fewer per pair.
  float p = fmaf(w, 1.0f / 3.0f, 0.4f);
  p = fmaf(w, p, 0.5f);
  p = fmaf(w, p, 2.0f / 3.0f);
  p = fmaf(w, p, 1.0f);
  p = fmaf(w, p, 2.0f);
  return w * p;
}

// -2 ln u1 on the log path.
TSDE_D float box_muller_log(uint32_t a) {
  const float u1 = fmaf((float)a, 0x1p-32f, 0x1p-33f);
  return -1.3862943611198906f * __builtin_amdgcn_logf(u1);  // -2 ln2 * log2(u1)
}

// One pair (normal1 and the one-element-per-lane paths): every lane evaluates both the log and the series.
TSDE_D void box_muller(uint32_t a, uint32_t b, float& n0, float& n1) {
  const float s_log = box_muller_log(a);
  const float s_ser = box_muller_series(a);
  const float s = (a >= kSeriesFrom) ? s_ser : s_log;
  const float r = __builtin_amdgcn_sqrtf(s);
  const float t = (float)b * 0x1p-32f;
  n0 = r * __builtin_amdgcn_cosf(t);
  n1 = r * __builtin_amdgcn_sinf(t);
}

// The small-radius series in its two factors: box_muller_series(a) = w * p.
TSDE_D void box_muller_series_factors(uint32_t a, float& w, float& p) {
  w = fmaf((float)(~a), 0x1p-32f, 0x1p-33f);
  p = fmaf(w, 1.0f / 3.0f, 0.4f);
  p = fmaf(w, p, 0.5f);
  p = fmaf(w, p, 2.0f / 3.0f);
  p = fmaf(w, p, 1.0f);
  p = fmaf(w, p, 2.0f);
}

// Radii times cos / sin of the two angles: the tail both two-pair forms share.
TSDE_D void box_muller2_finish(const u32x4& r, float s0, float s1, float (&n)[4]) {
  const float r0 = __builtin_amdgcn_sqrtf(s0);
  const float r1 = __builtin_amdgcn_sqrtf(s1);
  const float t0 = (float)r.y * 0x1p-32f;
  const float t1 = (float)r.w * 0x1p-32f;
  n[0] = r0 * __builtin_amdgcn_cosf(t0);
  n[1] = r0 * __builtin_amdgcn_sinf(t0);
  n[2] = r1 * __builtin_amdgcn_cosf(t1);
  n[3] = r1 * __builtin_amdgcn_sinf(t1);
}

// Both pairs of one Philox call, the series evaluated once, chosen by selects. The series value is kept for 1 pair in 16, so
// a lane needs it for both of its pairs only 1 time in 256: the lane evaluates it on whichever pair is hot (the first if both
// are), and the second pair of a both-hot lane is redone in a block that the wave enters only when some lane has one
// (1 - (255/256)^64 = 22 % of the draws of a full wave). The same floats as box_muller on each pair, bit for bit, by
// construction: a hot pair gets series(its own word) through the same operations in the same order, a cold pair its
// log value, and the selects only choose between those. Three vector compares and three v_cndmask_b32 per draw.
TSDE_D void box_muller2_selects(const u32x4& r, float (&n)[4]) {
  float s0 = box_muller_log(r.x);
  float s1 = box_muller_log(r.z);
  const bool h0 = r.x >= kSeriesFrom;
  const bool h1 = r.z >= kSeriesFrom;
  const float ser = box_muller_series(h0 ? r.x : r.z);
  s0 = h0 ? ser : s0;
  s1 = (h1 && !h0) ? ser : s1;
  if (__builtin_expect(__builtin_amdgcn_ballot_w64(h0 && h1) != 0, 0)) {
    asm volatile("" ::: "memory");   // keeps the block a branch: without it the compiler folds it back into selects
    s1 = (h0 && h1) ? box_muller_series(r.z) : s1;
  }
  box_muller2_finish(r, s0, s1, n);
}

// The same, with the results written under the execution mask instead of through selects. The two compares land in scalar
// registers as lane masks (ballots: a lane that is not active at entry -- the ragged last wave of a launch -- has a zero bit in
// both). The series runs on the first word where that is hot and on the second elsewhere (one v_cndmask_b32 on the first mask),
// and its final product w * p is written into s0 by the lanes of h0 and into s1 by the lanes of h1, each with its mask as the
// execution mask, which is then put back to its value at entry -- never to all ones. That leaves a both-hot lane with the
// first word's series in both radii; the block the wave enters on h0 & h1 != 0 (a scalar AND of the two masks; as before 22 %
// of a full wave's draws) evaluates the series of the second word and writes it into s1 under h0 & h1. Two vector compares,
// one v_cndmask_b32 and two v_mul_f32 where the select form has three, three and one; the cold block 9 vector instructions.
// Bit for bit box_muller on each pair, as above: the masked writes move the same w * p that the selects moved
// (tests/test_box_muller_select.py restates the selection, tests/test_gpu_box_muller_ragged.py runs it in ragged waves).
// Picking the series' word with v_max_u32 (a hot word is larger than any cold one) was built and measured slower: the cold
// block then has to find which pair holds the smaller word (profiles/bm_select_notes.txt).
TSDE_D void box_muller2(const u32x4& r, float (&n)[4]) {
  float s0 = box_muller_log(r.x);
  float s1 = box_muller_log(r.z);
  const uint64_t m0 = __builtin_amdgcn_ballot_w64(r.x >= kSeriesFrom);
  const uint64_t m1 = __builtin_amdgcn_ballot_w64(r.z >= kSeriesFrom);
  float w, p;
  box_muller_series_factors(r.x >= kSeriesFrom ? r.x : r.z, w, p);
  uint64_t entry;
  asm volatile(
      "s_mov_b64 %[entry], exec\n\t"
      "s_mov_b64 exec, %[m0]\n\t"
      "v_mul_f32_e32 %[s0], %[w], %[p]\n\t"
      "s_mov_b64 exec, %[m1]\n\t"
      "v_mul_f32_e32 %[s1], %[w], %[p]\n\t"
      "s_mov_b64 exec, %[entry]"
      : [s0] "+v"(s0), [s1] "+v"(s1), [entry] "=&s"(entry)
      : [w] "v"(w), [p] "v"(p), [m0] "s"(m0), [m1] "s"(m1));
  const uint64_t both = m0 & m1;
  if (__builtin_expect(both != 0, 0)) {
    asm volatile("" ::: "memory");   // keeps the block a branch: without it the compiler folds it back into selects
    box_muller_series_factors(r.z, w, p);
    asm volatile(
        "s_mov_b64 %[entry], exec\n\t"
        "s_mov_b64 exec, %[both]\n\t"
        "v_mul_f32_e32 %[s1], %[w], %[p]\n\t"
        "s_mov_b64 exec, %[entry]"
        : [s1] "+v"(s1), [entry] "=&s"(entry)
        : [w] "v"(w), [p] "v"(p), [both] "s"(both));
  }
  box_muller2_finish(r, s0, s1, n);
}

TSDE_D void box_muller(uint32_t a, uint32_t b, double& n0, double& n1) {
  const double u1 = ((double)a + 0.5) * 0x1p-32;
  const double r = sqrt(-2.0 * log(u1));
  double s, c;
  sincospi((double)b * 0x1p-31, &s, &c);
  n0 = r * c;
  n1 = r * s;
}

TSDE_D void box_muller2(const u32x4& r, double (&n)[4]) {
  box_muller(r.x, r.y, n[0], n[1]);
  box_muller(r.z, r.w, n[2], n[3]);
}

TSDE_D void box_muller2_selects(const u32x4& r, double (&n)[4]) { box_muller2(r, n); }

// Four standard normals of one (quad, cell, node, stream).
template <typename T>
TSDE_D void normal4(const NoiseKey& key, uint64_t quad, uint32_t cell, uint64_t node, uint32_t stream, T (&n)[4]) {
  const u32x4 r = noise_bits(key, quad, cell, node, stream);
  box_muller2(r, n);
}

// The same four normals through the select form of the shared series: the entry point of callers that the masked writes of
// box_muller2 cost scalar spills (the SRK step kernels of steps.hip: profiles/bm_select_resource_usage_notes.txt).
template <typename T>
TSDE_D void normal4_selects(const NoiseKey& key, uint64_t quad, uint32_t cell, uint64_t node, uint32_t stream, T (&n)[4]) {
  const u32x4 r = noise_bits(key, quad, cell, node, stream);
  box_muller2_selects(r, n);
}

// The same four normals with the series evaluated on both pairs: the entry point of callers whose register allocation the
// branch of box_muller2 upsets (scratch, spills or a lost wave of occupancy in profiles/bm_shared_series_resource_usage_*.txt:
// the matrix-core kernels, the general-noise step kernels and the SRK forms of the trajectory kernels).
template <typename T>
TSDE_D void normal4_pairs(const NoiseKey& key, uint64_t quad, uint32_t cell, uint64_t node, uint32_t stream, T (&n)[4]) {
  const u32x4 r = noise_bits(key, quad, cell, node, stream);
  box_muller(r.x, r.y, n[0], n[1]);
  box_muller(r.z, r.w, n[2], n[3]);
}

// Four CONSECUTIVE normals of the field from any global element index `elem` (not a multiple of 4 in general: the rows of
// a field whose row stride is no multiple of 4, the (B, d + 1) Brownian motion of a logqp solve): the two Philox quads
// the four elements straddle, selected by elem & 3. Element for element what normal1 returns. Twice the work of
// normal4_pairs; an aligned `elem` still draws both quads (the select is per lane, the draw is not).
template <typename T>
TSDE_D void normal4_straddle(const NoiseKey& key, uint64_t elem, uint32_t cell, uint64_t node, uint32_t stream, T (&n)[4]) {
  T lo[4], hi[4];
  normal4_pairs<T>(key, elem >> 2, cell, node, stream, lo);
  normal4_pairs<T>(key, (elem >> 2) + 1, cell, node, stream, hi);
  const uint32_t s = (uint32_t)elem & 3u;
  n[0] = s == 0 ? lo[0] : s == 1 ? lo[1] : s == 2 ? lo[2] : lo[3];
  n[1] = s == 0 ? lo[1] : s == 1 ? lo[2] : s == 2 ? lo[3] : hi[0];
  n[2] = s == 0 ? lo[2] : s == 1 ? lo[3] : s == 2 ? hi[0] : hi[1];
  n[3] = s == 0 ? lo[3] : s == 1 ? hi[0] : s == 2 ? hi[1] : hi[2];
}

// One standard normal for a single global element (generic / unaligned paths).
template <typename T>
TSDE_D T normal1(const NoiseKey& key, uint64_t elem, uint32_t cell, uint64_t node, uint32_t stream) {
  const u32x4 r = noise_bits(key, elem >> 2, cell, node, stream);
  const uint32_t lane = (uint32_t)elem & 3u;
  const uint32_t a = (lane & 2u) ? r.z : r.x;
  const uint32_t b = (lane & 2u) ? r.w : r.y;
  T n0, n1;
  box_muller(a, b, n0, n1);
  return (lane & 1u) ? n1 : n0;
}
// The draws of one solver step as the trajectory kernels' step loops make them: node 0 of `cell`, whose Philox head is
// the same for every lane and every stream (scalar work, once per step). Same normals as normal4 / normal1 with node = 0.
struct StepNoise {
  NoiseKey key;
  uint32_t cell;
  PhiloxHead head;
  TSDE_D StepNoise(const NoiseKey& k, uint32_t cell_) : key(k), cell(cell_), head(philox_head(cell_, 0u, k.k0)) {}
  TSDE_D u32x4 bits(uint64_t quad, uint32_t stream) const {
    return philox4x32_10_headed(noise_counter(quad, cell, 0, stream), key.k0, key.k1, head);
  }
  template <typename T>
  TSDE_D void normal4(uint64_t quad, uint32_t stream, T (&n)[4]) const {
    const u32x4 r = bits(quad, stream);
    box_muller2(r, n);
  }
  template <typename T>
  TSDE_D void normal4_pairs(uint64_t quad, uint32_t stream, T (&n)[4]) const {
    const u32x4 r = bits(quad, stream);
    box_muller(r.x, r.y, n[0], n[1]);
    box_muller(r.z, r.w, n[2], n[3]);
  }
  template <typename T>
  TSDE_D T normal1(uint64_t elem, uint32_t stream) const {
    const u32x4 r = bits(elem >> 2, stream);
    const uint32_t lane = (uint32_t)elem & 3u;
    const uint32_t a = (lane & 2u) ? r.z : r.x;
    const uint32_t b = (lane & 2u) ? r.w : r.y;
    T n0, n1;
    box_muller(a, b, n0, n1);
    return (lane & 1u) ? n1 : n0;
  }
};

// The same three draws through the free functions above, nothing precomputed: the source of the step loops that have not
// moved onto the shared Philox head.
struct PlainStepNoise {
  NoiseKey key;
  uint32_t cell;
  TSDE_D PlainStepNoise(const NoiseKey& k, uint32_t cell_) : key(k), cell(cell_) {}
  template <typename T>
  TSDE_D void normal4(uint64_t quad, uint32_t stream, T (&n)[4]) const { tsde::normal4<T>(key, quad, cell, 0, stream, n); }
  template <typename T>
  TSDE_D void normal4_pairs(uint64_t quad, uint32_t stream, T (&n)[4]) const {
    tsde::normal4_pairs<T>(key, quad, cell, 0, stream, n);
  }
  template <typename T>
  TSDE_D T normal1(uint64_t elem, uint32_t stream) const { return tsde::normal1<T>(key, elem, cell, 0, stream); }
};
#endif  // __HIPCC__

}  // namespace tsde
