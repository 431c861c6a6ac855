// The fused uniform-sample + minibatch-gather + whitening-statistics pass as a device function (replay_memory.py:123-138 +
// base_network.py:95-96): gather_stats_kernel (replay.hip) is a wrapper around it, and so are the launches it shares with another
// kernel (reduce_gather_kernel, conv1_dw_gather_kernel).  The caller provides its LDS: sh [256 * GATHER_SH] floats, dsh
// [CPP_MAX_CHANNELS * 16] doubles, lut [256] floats.
//
// The sums are EXACT for pixel states (round 4): var = E[x^2] - mu^2 cancels 20-80 x on a render's near-constant channels (a sky, a
// floor), where the f32 per-lane chains of rounds 1-3 (36 terms each, 1e-7 relative) moved the whitening scale by 2e-6 relative --
// 5e-5 absolute on conv1 outputs of magnitude 13 (profiles/experiments/r04_render_probe.txt).  A lane now carries both sums in f64 (the square of an f16 has 22 bits, a
// lane adds <= ~10^2 of them: exact); they cross LDS as (hi, lo) float pairs and are combined in f64 as before.
#pragma once
#include "common.h"
constexpr int GATHER_SH = 16;      // floats per thread: (hi, lo) of one statistic's 8 element sums
constexpr int GATHER_LDS_BYTES = 256 * GATHER_SH * 4 + CPP_MAX_CHANNELS * 16 * 8 + 256 * 4;

__device__ __forceinline__ int sample_row(uint64_t seed, uint64_t counter, int b, int size) {
  u32x4 c = {(uint32_t)b, 0u, (uint32_t)counter, (uint32_t)(counter >> 32)};
  const u32x4 r = philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  return (int)(((uint64_t)r.x * (uint64_t)size) >> 32);      // uniform in [0, size)
}

template <typename T> struct Vec8;
template <> struct Vec8<__half> {
  typedef __half Out;
  uint4 raw;
  __device__ void load(const __half* p) { raw = *reinterpret_cast<const uint4*>(p); }
  __device__ void store(__half* p) const { *reinterpret_cast<uint4*>(p) = raw; }
  __device__ float get(int e) const {
    const uint32_t w = e < 2 ? raw.x : (e < 4 ? raw.y : (e < 6 ? raw.z : raw.w));
    const unsigned short h = (e & 1) ? (unsigned short)(w >> 16) : (unsigned short)(w & 0xffffu);
    return __half2float(__ushort_as_half(h));
  }
};
// 8-bit pixel codes (CPP_U8 store): 8 codes per vector, looked up in the f16(k/255) table (LDS copy); gathered as f16
template <> struct Vec8<uint8_t> {
  typedef __half Out;
  uint2 raw; const float* lut;
  __device__ void load(const uint8_t* p) { raw = *reinterpret_cast<const uint2*>(p); }
  __device__ float get(int e) const { return lut[((e < 4 ? raw.x : raw.y) >> (8 * (e & 3))) & 0xffu]; }
  __device__ void store(__half* p) const {
    uint4 o;
    uint32_t* w = reinterpret_cast<uint32_t*>(&o);
#pragma unroll
    for (int e = 0; e < 8; e += 2)
      w[e >> 1] = (uint32_t)__half_as_ushort(__float2half(get(e))) | ((uint32_t)__half_as_ushort(__float2half(get(e + 1))) << 16);
    *reinterpret_cast<uint4*>(p) = o;
  }
};
template <> struct Vec8<float> {
  typedef float Out;
  float4 a, b;
  __device__ void load(const float* p) {
    a = *reinterpret_cast<const float4*>(p); b = *reinterpret_cast<const float4*>(p + 4);
  }
  __device__ void store(float* p) const {
    *reinterpret_cast<float4*>(p) = a; *reinterpret_cast<float4*>(p + 4) = b;
  }
  __device__ float get(int e) const {
    switch (e) { case 0: return a.x; case 1: return a.y; case 2: return a.z; case 3: return a.w;
                 case 4: return b.x; case 5: return b.y; case 6: return b.z; default: return b.w; }
  }
};

template <typename V> __device__ __forceinline__ void vec_init(V&, const float*) {}
__device__ __forceinline__ void vec_init(Vec8<uint8_t>& v, const float* lut) { v.lut = lut; }
template <typename T, typename O> __device__ __forceinline__ O elem_convert(T x, const float*) { return (O)x; }
template <> __device__ __forceinline__ __half elem_convert<uint8_t, __half>(uint8_t k, const float* lut) { return __float2half(lut[k]); }

__host__ __device__ inline int gcd_int(int a, int b) { while (b) { int t = a % b; a = b; b = t; } return a; }

// f32 product / sum, each rounded on its own: never contracted into an FMA (the n-step return's fixed operation order, which the
// host's numpy restatement in replay_memory.py repeats bit for bit)
__device__ __forceinline__ float nstep_mul(float x, float y) {
#pragma clang fp contract(off)
  return x * y;
}
__device__ __forceinline__ float nstep_add(float x, float y) {
#pragma clang fp contract(off)
  return x + y;
}

// n-step walk (include/cartpolepp_abi.h, "n-step returns"), by every lane of a wave for the wave-uniform drawn row i: lane k < n loads
// the four columns of row j_k = (i + k) mod R in ONE round of loads (the only memory trip between the row and the state's slot, as the
// uniform gather's row -> slot load); lane k links to k + 1 if mask[j_k] != 0, row j_{k+1} exists (j_k + 1 < size, or the memory is
// full and j_{k+1} != i) and s2_idx[j_k] == s1_idx[j_{k+1}].  The first lane that does not link is the last row walked, m - 1.
// which == 1: the slot of s2_idx[j_{m-1}]; which == 0: the slot of s1_idx[i] and the folded reward / mask, added in the fixed order
// g_k = g_{k-1} * discount, R_k = R_{k-1} + r[j_k] * g_k, mask = mask[j_{m-1}] * g_{m-1} (n = 1: the stored values).
__device__ __forceinline__ void nstep_walk(const GatherArgs& a, const int row, const int which, const int lane, int* slot, float* reward,
                                           float* mask) {
  const int n = a.nstep->n;
  const float discount = a.nstep->discount;
  const int size = a.size_ptr ? *a.size_ptr : a.size, R = a.rows_cap;
  const bool full = size >= R;
  const bool have = lane < n && (full ? lane < R : row + lane < size);      // (row < size <= R: every j below is a row of the memory)
  const int j = full ? (row + lane) % R : row + lane;
  float m = 0.f, r = 0.f; int s1 = -1, s2 = -1;
  if (have) { m = a.mask[j]; r = a.reward[j]; s1 = a.s_idx[0][j]; s2 = a.s_idx[1][j]; }
  const int s1_next = __shfl_down(s1, 1);
  const bool have_next = __shfl_down((int)have, 1) != 0 && lane < 63;
  const bool link = have && m != 0.f && have_next && s2 == s1_next;
  const int last = __ffsll((unsigned long long)__ballot(!link)) - 1;        // (lane n - 1 never links: 0 <= last < n)
  if (which == 1) { *slot = __builtin_amdgcn_readlane(s2, last); return; }
  *slot = __builtin_amdgcn_readlane(s1, 0);
  float g = 1.f, ret = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(r), 0));
  for (int k = 1; k <= last; ++k) {
    g = nstep_mul(g, discount);
    ret = nstep_add(ret, nstep_mul(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(r), k)), g));
  }
  *reward = ret;
  *mask = nstep_mul(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(m), last)), g);
}

// ---- random shift (include/cartpolepp_abi.h, "Random shift"): out[y, x, c] = in[clamp(y + dy), clamp(x + dx), c] ------------------
// An output vector (8 elements, 16-byte aligned in the gathered copy) that lies inside one image row and whose 8 source elements are
// all inside the source row is 8 CONTIGUOUS source elements at element offset clamp(y + dy) * L + x0 + dx * C (L = W * C elements per
// row) -- 2-byte aligned in general, not 16.  It is read as the two ALIGNED vectors that cover it and realigned in registers: a mux by
// the dword part of the offset, then one v_alignbit per output dword for the sub-dword part.  The other vectors -- the |dx| pixels at
// one end of a row that repeat the edge pixel, and vectors that straddle two rows when L % 8 != 0 -- take their 8 elements one by one
// (`slow`); their loads are issued with the batch's, not behind it.  The lane -> channel-class structure is the output's, i.e. the
// unshifted gather's: a lane's vectors still hold the same 8 channels, so the statistics below are untouched.
template <typename T> struct ShiftElem { typedef uint16_t E; };
template <> struct ShiftElem<uint8_t> { typedef uint8_t E; };
struct ShiftGeom { int L, H, C, dy, dxC, ch[8]; long nvec; };      // ch[e]: channel of a lane's element e (the same for all its vectors)

template <typename T> struct ShiftVec {
  static constexpr int NW = (int)sizeof(T) * 2;      // dwords per vector of 8 elements
  uint32_t w[2 * NW];                                // the two aligned vectors that cover the source elements
  uint32_t el[8];                                    // slow: the 8 source elements
  int t; bool slow;

  __device__ __forceinline__ void issue(const T* src, const ShiftGeom& g, const long v) {
    const unsigned e0 = (unsigned)v * 8u;
    const int y = (int)(e0 / (unsigned)g.L), xe0 = (int)e0 - y * g.L;
    const int s0 = xe0 + g.dxC;
    slow = (xe0 + 8 > g.L) | (s0 < 0) | (s0 + 8 > g.L);
    const int sy = min(max(y + g.dy, 0), g.H - 1);
    const int base = slow ? 0 : sy * g.L + s0;
    t = base & 7;
    const long v0 = base >> 3, v1 = v0 + 1 < g.nvec ? v0 + 1 : v0;      // (v1 is read only when t != 0: then it is inside the state)
    if constexpr (NW == 4) {
      const uint4 lo = *reinterpret_cast<const uint4*>(src + v0 * 8), hi = *reinterpret_cast<const uint4*>(src + v1 * 8);
      w[0] = lo.x; w[1] = lo.y; w[2] = lo.z; w[3] = lo.w; w[NW] = hi.x; w[NW + 1] = hi.y; w[2 * NW - 2] = hi.z; w[2 * NW - 1] = hi.w;
    } else {
      const uint2 lo = *reinterpret_cast<const uint2*>(src + v0 * 8), hi = *reinterpret_cast<const uint2*>(src + v1 * 8);
      w[0] = lo.x; w[1] = lo.y; w[NW] = hi.x; w[NW + 1] = hi.y;
    }
    if (slow) {
      const typename ShiftElem<T>::E* s = reinterpret_cast<const typename ShiftElem<T>::E*>(src);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        int xe = xe0 + e, yy = y;
        if (xe >= g.L) { xe -= g.L; ++yy; }                     // (L >= 8: at most one row further; 8 v + e < elems: yy < H)
        const int c = g.ch[e];                                  // the element's channel (L % C == 0)
        const int xs = xe + g.dxC;
        const int col = xs < 0 ? c : (xs >= g.L ? g.L - g.C + c : xs);
        el[e] = (uint32_t)s[(long)min(max(yy + g.dy, 0), g.H - 1) * g.L + col];
      }
    }
  }

  __device__ __forceinline__ void finish(Vec8<T>& x) const {
    uint32_t o[NW];
    if (slow) {
#pragma unroll
      for (int j = 0; j < NW; ++j)
        o[j] = NW == 4 ? (el[2 * j] | (el[2 * j + 1] << 16))
                       : (el[(4 * j) & 7] | (el[(4 * j + 1) & 7] << 8) | (el[(4 * j + 2) & 7] << 16) | (el[(4 * j + 3) & 7] << 24));
    } else {
      const int tb = t * (int)sizeof(T), k = tb >> 2;          // byte offset inside the first vector: dword part, sub-dword part
      const uint32_t bits = (uint32_t)(tb & 3) * 8u;
      // (the mux as bit selects, v_bfi_b32: written as a choice between two array elements the compiler turns it into ONE load at a
      // run-time index, which puts the whole window into scratch memory)
      const uint32_t k1 = 0u - (uint32_t)(k & 1), k2 = 0u - (uint32_t)((k >> 1) & 1);
      uint32_t m[NW + 1];
      if constexpr (NW == 4) {
        uint32_t u[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) u[i] = (w[i + 2] & k2) | (w[i] & ~k2);
#pragma unroll
        for (int i = 0; i < 5; ++i) m[i] = (u[i + 1] & k1) | (u[i] & ~k1);
      } else {
#pragma unroll
        for (int i = 0; i < NW + 1; ++i) m[i] = (w[i + 1] & k1) | (w[i] & ~k1);
      }
#pragma unroll
      for (int j = 0; j < NW; ++j) o[j] = __builtin_amdgcn_alignbit(m[j + 1], m[j], bits);
    }
    set_raw(x, o);
  }
  static __device__ __forceinline__ void set_raw(Vec8<__half>& x, const uint32_t* o) { x.raw = make_uint4(o[0], o[1], o[2], o[3]); }
  static __device__ __forceinline__ void set_raw(Vec8<uint8_t>& x, const uint32_t* o) { x.raw = make_uint2(o[0], o[1]); }
};

// The (dy, dx) of gathered state (b, which) and the augmentation counter's advance.  Thread 0 of the workgroup reads the counter n,
// draws r = philox4x32_10({b, 2 + which, n_lo, n_hi}, seed) and takes a ticket (release: the read is complete before the ticket
// counts); the workgroup that takes the last of the launch's 2 B tickets writes n + 1 and clears the tickets.  Nobody reads the counter
// after its own ticket, so every workgroup of the launch has read n before n + 1 is written; the next gather is a later launch on the
// stream.  `shw`: two ints of LDS nothing else touches before the barrier below.
__device__ __forceinline__ void shift_draw(const GatherArgs& a, const int b, const int which, int* shw, int* dy, int* dx) {
  if (threadIdx.x == 0) {
    const uint64_t n = __hip_atomic_load(&a.shift->counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    u32x4 c = {(uint32_t)b, 2u + (uint32_t)which, (uint32_t)n, (uint32_t)(n >> 32)};
    const u32x4 r = philox4x32_10(c, (uint32_t)a.shift_seed, (uint32_t)(a.shift_seed >> 32));
    const uint64_t span = 2u * (uint32_t)a.shift_pad + 1u;
    const int y = (int)(((uint64_t)r.x * span) >> 32) - a.shift_pad, x = (int)(((uint64_t)r.y * span) >> 32) - a.shift_pad;
    shw[0] = y; shw[1] = x;
    a.shifts_out[((long)which * a.B + b) * 2] = y; a.shifts_out[((long)which * a.B + b) * 2 + 1] = x;
    const uint32_t ticket = __hip_atomic_fetch_add(&a.shift->ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (ticket == 2u * (uint32_t)a.B - 1u) {
      __hip_atomic_store(&a.shift->counter, n + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&a.shift->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  __syncthreads();
  *dy = shw[0]; *dx = shw[1];
}

// (b, which): the workgroup's place in the (B, 2) grid -- blockIdx for a launch of its own.  NSTEP: the memory's n-step instance
// (GatherArgs::nstep non-null); the uniform instances (false) compile to the instructions they had before the walk existed.  SHIFT: the
// random-shift instance (GatherArgs::shift non-null; a materialising pixel gather: out_state set, C > 0), likewise.
template <typename T, bool NSTEP = false, bool SHIFT = false>
__device__ __forceinline__ void gather_stats_body(const GatherArgs& a, const int b, const int which, float* sh, double* dsh, float* lut) {
  // (lut: CPP_U8 store, f16(k/255) as float)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr bool U8 = sizeof(T) == 1;
  if (U8) { lut[tid] = __half2float(a.lut[tid]); __syncthreads(); }
  typedef typename Vec8<T>::Out OutT;

  // --- sample + double indirection on lane 0, broadcast by wavefront shuffle
  int row = 0, slot = 0;
  if (lane == 0) {
    if (a.s_idx[0] == nullptr) { row = b; slot = b; }       // statistics over an already gathered batch
    else {
      row = a.rows ? a.rows[b] : sample_row(a.seed, (a.counter ? *a.counter : 0) + (uint64_t)a.counter_add, b, a.size_ptr ? *a.size_ptr : a.size);
      if (!NSTEP) slot = a.s_idx[which][row];
    }
  }
  row = __shfl(row, 0);
  slot = __shfl(slot, 0);
  float nreward = 0.f, nmask = 0.f;
  if (NSTEP && a.s_idx[0] != nullptr) nstep_walk(a, row, which, lane, &slot, &nreward, &nmask);
  int shift_dy = 0, shift_dx = 0;
  if constexpr (SHIFT) shift_draw(a, b, which, reinterpret_cast<int*>(dsh), &shift_dy, &shift_dx);

  if (tid == 0 && a.out_slot[which]) a.out_slot[which][b] = slot;
  if (which == 0 && a.s_idx[0] != nullptr) {
    if (tid == 0 && a.rows_out) a.rows_out[b] = row;
    if (tid < a.action_dim) a.out_action[(long)b * a.action_dim + tid] = a.action[(long)row * a.action_dim + tid];
    if (tid == 64) a.out_reward[b] = NSTEP ? nreward : a.reward[row];
    if (tid == 65) a.out_mask[b] = NSTEP ? nmask : a.mask[row];
  }

  const T* src = (const T*)a.store[which] + (long)slot * a.elems;
  OutT* dst = a.out_state[which] ? (OutT*)a.out_state[which] + (long)b * a.elems : nullptr;
  const long nvec = a.elems >> 3;
  const int C = a.C;

  // The store already holds this state's sums (computed by this same function when the state was written: launch_slot_stats) and
  // nobody wants a copy of the pixels (conv1 reads the store through out_slot): the sampled row costs 2 C doubles, not the image.
  if (a.slot_stats != nullptr && dst == nullptr && C > 0) {
    if (tid < 2 * C) a.part[((long)which * a.B + b) * 2 * C + tid] = a.slot_stats[(long)slot * 2 * C + tid];
    return;
  }

  if (C <= 0) {                                   // gather only (low-dim states)
    for (long v = tid; v < nvec; v += 256) { Vec8<T> x; vec_init(x, lut); x.load(src + v * 8); if (dst) x.store(dst + v * 8); }
    for (long e = nvec * 8 + tid; e < a.elems; e += 256) if (dst) dst[e] = elem_convert<T, OutT>(src[e], lut);
    return;
  }

  const int P = C / gcd_int(8, C);
  const int act = (64 / P) * P;                   // lanes in use per wave: multiple of the period
  double s[8], ss[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { s[e] = 0.0; ss[e] = 0.0; }
  if constexpr (SHIFT) {
    if (lane < act) {
      // as the loop below: GU output vectors per thread in flight (two aligned loads each), the same vectors per lane in the same order
      constexpr int GU = 6;
      ShiftGeom g;
      g.L = a.shift_W * a.shift_C; g.H = a.shift_H; g.C = a.shift_C; g.dy = shift_dy; g.dxC = shift_dx * a.shift_C; g.nvec = nvec;
#pragma unroll
      for (int e = 0; e < 8; ++e) g.ch[e] = (8 * (wave * act + lane) + e) % a.shift_C;
      long v = wave * act + lane;
      const long stride = 4 * act;
      for (; v + (GU - 1) * stride < nvec; v += GU * stride) {
        ShiftVec<T> s0, s1, s2, s3, s4, s5;       // (named, not an array: each stays in registers)
        static_assert(GU == 6, "one ShiftVec per vector in flight");
        s0.issue(src, g, v); s1.issue(src, g, v + stride); s2.issue(src, g, v + 2 * stride);
        s3.issue(src, g, v + 3 * stride); s4.issue(src, g, v + 4 * stride); s5.issue(src, g, v + 5 * stride);
        auto finish = [&](const ShiftVec<T>& sv, const long vo) __attribute__((always_inline)) {
          Vec8<T> x;
          vec_init(x, lut);
          sv.finish(x);
          x.store(dst + vo * 8);
#pragma unroll
          for (int e = 0; e < 8; ++e) { const double f = (double)x.get(e); s[e] += f; ss[e] = fma(f, f, ss[e]); }
        };
        finish(s0, v); finish(s1, v + stride); finish(s2, v + 2 * stride);
        finish(s3, v + 3 * stride); finish(s4, v + 4 * stride); finish(s5, v + 5 * stride);
      }
      for (; v < nvec; v += stride) {
        ShiftVec<T> sv;
        sv.issue(src, g, v);
        Vec8<T> x;
        vec_init(x, lut);
        sv.finish(x);
        x.store(dst + v * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) { const double f = (double)x.get(e); s[e] += f; ss[e] = fma(f, f, ss[e]); }
      }
    }
  } else if (lane < act) {
    // GU row vectors per thread in flight (one 16-byte load each is far too little to cover the HBM latency with two
    // workgroups per CU); the accumulation order per lane is unchanged
    constexpr int GU = 6;
    long v = wave * act + lane;
    const long stride = 4 * act;
    for (; v + (GU - 1) * stride < nvec; v += GU * stride) {
      Vec8<T> x[GU];
#pragma unroll
      for (int u = 0; u < GU; ++u) { vec_init(x[u], lut); x[u].load(src + (v + u * stride) * 8); }
#pragma unroll
      for (int u = 0; u < GU; ++u) {
        if (dst) x[u].store(dst + (v + u * stride) * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) { const double f = (double)x[u].get(e); s[e] += f; ss[e] = fma(f, f, ss[e]); }
      }
    }
    for (; v < nvec; v += stride) {
      Vec8<T> x;
      vec_init(x, lut);
      x.load(src + v * 8);
      if (dst) x.store(dst + v * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) { const double f = (double)x.get(e); s[e] += f; ss[e] = fma(f, f, ss[e]); }
    }
  }
  // stage 2: per (class q, element e): sum the lanes of that class over the 4 waves, in f64.  One statistic at a time, each f64
  // lane sum crossing LDS as a (hi, lo) float pair (48 bits of a sum of <= ~10^2 terms of <= 22 bits: nothing is lost)
#pragma unroll
  for (int stat = 0; stat < 2; ++stat) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const double v = stat ? ss[e] : s[e];
      const float hi = (float)v;
      sh[tid * GATHER_SH + e] = hi; sh[tid * GATHER_SH + 8 + e] = (float)(v - (double)hi);
    }
    __syncthreads();
    if (tid < P * 8) {
      const int q = tid >> 3, e = tid & 7;
      double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;    // one chain per wave: four LDS reads in flight instead of one
      for (int l = q; l < act; l += P) {
        a0 += (double)sh[(0 * 64 + l) * GATHER_SH + e] + (double)sh[(0 * 64 + l) * GATHER_SH + 8 + e];
        a1 += (double)sh[(1 * 64 + l) * GATHER_SH + e] + (double)sh[(1 * 64 + l) * GATHER_SH + 8 + e];
        a2 += (double)sh[(2 * 64 + l) * GATHER_SH + e] + (double)sh[(2 * 64 + l) * GATHER_SH + 8 + e];
        a3 += (double)sh[(3 * 64 + l) * GATHER_SH + e] + (double)sh[(3 * 64 + l) * GATHER_SH + 8 + e];
      }
      dsh[q * 16 + stat * 8 + e] = (a0 + a1) + (a2 + a3);
    }
    __syncthreads();
  }
  // stage 3: per channel: the (q, e) pairs with (8q + e) % C == c
  if (tid < 2 * C) {
    const int stat = tid / C, c = tid - stat * C;
    double acc = 0.0;
    for (int q = 0; q < P; ++q) {                  // elements e of class q with (8 q + e) % C == c, ascending
      int e = (c - 8 * q) % C; if (e < 0) e += C;
      for (; e < 8; e += C) acc += dsh[q * 16 + stat * 8 + e];
    }
    a.part[((long)which * a.B + b) * 2 * C + tid] = acc;
  }
}

