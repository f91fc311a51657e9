// odk_lanes.h -- one wavefront's lanes working together: the LDS hand-off barrier (ODK_SYNC), the phase-timing / phase-marker switch
// (ODK_PROF, ODK_PROF_BEGIN, ODK_LS_LOOP), and the cross-lane DPP reductions, row shifts, ordered keys and broadcasts.  The report kernels
// (odk_reports.hip) take ODK_DPP from here.  Bottom layer: stands on the HIP runtime header alone.
#pragma once
#include <hip/hip_runtime.h>

namespace odk {

// One workgroup == one wavefront: DS (LDS) instructions of a wave are issued and serviced in order, so
// cross-lane hand-offs through LDS need no s_barrier and no s_waitcnt -- only a compiler barrier that keeps
// the LDS accesses in program order (and stops values being cached in registers across the hand-off).
// NOTE: never put __restrict__ on an LDS pointer: with noalias the optimiser may treat the barrier as not
// touching that memory and reuse a value loaded before another lane's store.
#define ODK_SYNC() asm volatile("" ::: "memory")

// Phase timing (build with -DODK_PROFILE): lane 0 accumulates shader-clock deltas per phase into the
// scratch area, which the debug LDS image carries out.  Zero cost when the macro is off.
#ifdef ODK_PROFILE
#define ODK_PROF(i) do { if (lane == 0) { long long _t = clock64(); SCR[S::S_PROF + (i)] += (float)(_t - _tprev); _tprev = _t; } } while (0)
#define ODK_PROF_BEGIN() long long _tprev = clock64()
#define ODK_LS_LOOP(tag) do { if (lane == 0 && (tag) == 0) SCR[S::S_PROF3] += 1.0f; } while (0)   // one pass of the line search's bracketing loop
#elif defined(ODK_MARK)   // phase markers in the ISA listing (tools/isa_phase_stats.py): comments only
#define ODK_PROF(i) asm volatile("; ODK_PHASE_END " #i ::: "memory")
#define ODK_PROF_BEGIN() asm volatile("; ODK_PHASE_BEGIN" ::: "memory")
#define ODK_LS_LOOP(tag) asm volatile("; LS_LOOP_" #tag ::: "memory")   // LS_LOOP_0 .. LS_LOOP_1: the loop body as a region of its own (tools/isa_select_census.py)
#else
#define ODK_PROF(i) do { } while (0)
#define ODK_PROF_BEGIN() do { } while (0)
#define ODK_LS_LOOP(tag) do { } while (0)
#endif

// ------------------------------------------------------------------------------------------------
// Cross-lane all-reduce over the G lanes of one env with DPP (no LDS traffic): xor-1 / xor-2 quad permutes,
// row_half_mirror, row_mirror give every lane its 16-lane row total; rows are then combined with row_bcast15
// (/31) and the group total is read back with v_readlane.  MUST be called in uniform control flow.
// old = 0 with bound_ctrl lets the compiler fold the permute into the consuming VALU op (v_add_f32_dpp ...): one
// instruction per butterfly stage, no copies, no hazard nops.  (All four patterns read only enabled in-row lanes.)
#define ODK_DPP(v, ctrl, rmask) __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), ctrl, rmask, 0xF, true))
struct OpSum { static __device__ __forceinline__ float f(float a, float b) { return a + b; } };
struct OpMax { static __device__ __forceinline__ float f(float a, float b) { return fmaxf(a, b); } };
struct OpMin { static __device__ __forceinline__ float f(float a, float b) { return fminf(a, b); } };
typedef unsigned int odk_u2 __attribute__((ext_vector_type(2)));
template <int G, class Op> __device__ __forceinline__ float greduce(float v) {
  v = Op::f(v, ODK_DPP(v, 0xB1, 0xF));    // quad_perm [1,0,3,2]
  v = Op::f(v, ODK_DPP(v, 0x4E, 0xF));    // quad_perm [2,3,0,1]
  v = Op::f(v, ODK_DPP(v, 0x141, 0xF));   // row_half_mirror
  v = Op::f(v, ODK_DPP(v, 0x140, 0xF));   // row_mirror: every lane holds its row's total
  // gfx950 v_permlane16_swap: rows (r0 r1 r2 r3),(s0 s1 s2 s3) -> (r0 s0 r2 s2),(r1 s1 r3 s3); with both operands = v the
  // two results are (x0 x0 x2 x2) and (x1 x1 x3 x3): their combination is the 32-lane group total in every lane.
  const unsigned iv = __float_as_uint(v);
  const odk_u2 h = __builtin_amdgcn_permlane16_swap(iv, iv, false, false);
  v = Op::f(__uint_as_float(h[0]), __uint_as_float(h[1]));
  if (G == 64) {   // v_permlane32_swap: halves (lo hi),(lo hi) -> (lo lo),(hi hi)
    const unsigned iw = __float_as_uint(v);
    const odk_u2 w = __builtin_amdgcn_permlane32_swap(iw, iw, false, false);
    v = Op::f(__uint_as_float(w[0]), __uint_as_float(w[1]));
  }
  return v;
}
template <int G> __device__ __forceinline__ float gsum(float v) { return greduce<G, OpSum>(v); }
// Chain scans of forward_env (P1 / P2), step si = 0, 1, 2 shifts by 2^si lanes: row_shr (lane l reads lane l - 2^si) and
// row_shl (l + 2^si) inside the lane's 16-lane row, 0 from beyond the row's edge (bound_ctrl).  The host's body-to-lane
// layout keeps every serial body chain inside one row.  Uniform control flow only; si must fold to a constant.
__device__ __forceinline__ float row_shr(float v, int si) { return si == 0 ? ODK_DPP(v, 0x111, 0xF) : si == 1 ? ODK_DPP(v, 0x112, 0xF) : ODK_DPP(v, 0x114, 0xF); }
__device__ __forceinline__ float row_shl(float v, int si) { return si == 0 ? ODK_DPP(v, 0x101, 0xF) : si == 1 ? ODK_DPP(v, 0x102, 0xF) : ODK_DPP(v, 0x104, 0xF); }
// N sums at once (G = 32): the four in-row butterfly stages on the VALU as above, then the two rows are exchanged by
// ds_swizzle (xor 16 inside each 32-lane group: the LDS crossbar, no memory access and no VALU slot) instead of
// v_permlane16_swap (~8 cycles of VALU issue each); the N swizzles are in flight together, so their latency is paid once.
template <int G, int N> __device__ __forceinline__ void gsum_n(float* v) {
  if constexpr (G == 32) {
    float o[N];
#pragma unroll
    for (int i = 0; i < N; i++) {
      float x = v[i];
      x += ODK_DPP(x, 0xB1, 0xF); x += ODK_DPP(x, 0x4E, 0xF); x += ODK_DPP(x, 0x141, 0xF); x += ODK_DPP(x, 0x140, 0xF);
      v[i] = x;
      o[i] = __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(x), 0x401F));   // bit mode: and 0x1F, or 0, xor 0x10
    }
#pragma unroll
    for (int i = 0; i < N; i++) v[i] += o[i];
  } else {
#pragma unroll
    for (int i = 0; i < N; i++) v[i] = gsum<G>(v[i]);
  }
}
// max / min / argmax run on order-preserving unsigned keys: integer v_max_u32 / v_min_u32 fold the DPP permute into the
// op (float max needs a canonicalising v_max x, x per stage under IEEE mode, and then the permute stays a separate mov)
__device__ __forceinline__ unsigned fkey(float v) { const unsigned b = __float_as_uint(v); return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
__device__ __forceinline__ float fkey_inv(unsigned k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu)); }
#define ODK_DPPU(v, ctrl) ((unsigned)__builtin_amdgcn_update_dpp(0, (int)(v), ctrl, 0xF, 0xF, true))
template <int G, bool MAX> __device__ __forceinline__ unsigned greduce_u(unsigned v) {
  auto op = [](unsigned a, unsigned b) { return MAX ? (a > b ? a : b) : (a < b ? a : b); };
  v = op(v, ODK_DPPU(v, 0xB1));
  v = op(v, ODK_DPPU(v, 0x4E));
  v = op(v, ODK_DPPU(v, 0x141));
  v = op(v, ODK_DPPU(v, 0x140));
  const odk_u2 h = __builtin_amdgcn_permlane16_swap(v, v, false, false);
  v = op(h[0], h[1]);
  if (G == 64) {
    const odk_u2 w = __builtin_amdgcn_permlane32_swap(v, v, false, false);
    v = op(w[0], w[1]);
  }
  return v;
}
template <int G> __device__ __forceinline__ float gmax(float v) { return fkey_inv(greduce_u<G, true>(fkey(v))); }
template <int G> __device__ __forceinline__ float gmin(float v) { return fkey_inv(greduce_u<G, false>(fkey(v))); }
// argmax, lowest index wins ties (jnp.argmax semantics): max of the values, then min index among the maxima
template <int G> __device__ __forceinline__ int gargmax(float v, int i) {
  const unsigned k = fkey(v);
  const unsigned mx = greduce_u<G, true>(k);
  return (int)greduce_u<G, false>(k == mx ? (unsigned)i : 0x7FFFFFFFu);
}
// value held by lane j (uniform j < G) of this env's lane group, via v_readlane (no LDS)
template <int G> __device__ __forceinline__ float bcast(float v, int j) {
  const int iv = __float_as_int(v);
  if (G == 64) return __int_as_float(__builtin_amdgcn_readlane(iv, j));
  const int lo = __builtin_amdgcn_readlane(iv, j), hi = __builtin_amdgcn_readlane(iv, j + 32);
  return __int_as_float((threadIdx.x & 32) ? hi : lo);
}
// uniform integer static of lane j (identical in every env of the wave)
__device__ __forceinline__ int ubcast(int v, int j) { return __builtin_amdgcn_readlane(v, j); }

// 16-lane row reductions on unsigned keys (the first four butterfly stages of greduce_u: every lane ends with its row's value)
template <bool MAX> __device__ __forceinline__ unsigned rreduce_u(unsigned v) {
  auto op = [](unsigned a, unsigned b) { return MAX ? (a > b ? a : b) : (a < b ? a : b); };
  v = op(v, ODK_DPPU(v, 0xB1));
  v = op(v, ODK_DPPU(v, 0x4E));
  v = op(v, ODK_DPPU(v, 0x141));
  v = op(v, ODK_DPPU(v, 0x140));
  return v;
}

}  // namespace odk
