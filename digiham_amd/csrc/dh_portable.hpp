// dh_portable.hpp -- how the kernel bodies are written.
//
// Every kernel in this library is "one channel (or one small group of codewords) per
// 64-lane wavefront", one wavefront per workgroup.  The bodies are written as a sequence of
// PHASES: inside a phase each lane works independently (DH_FOR_LANES), between phases the
// lanes exchange data through the workgroup's LDS block and meet at DH_BARRIER().  Wave-wide
// votes use DH_BALLOT_ACC.  Loop control between phases only uses wave-uniform values.
//
// When hipcc compiles this for gfx950, DH_FOR_LANES binds `lane` to threadIdx.x, DH_BARRIER is
// s_barrier (free for a single-wave workgroup apart from the LDS wait) and DH_BALLOT_ACC is
// v_cmp + s_mov of the EXEC-wide vote.  When a plain C++ compiler builds the *test harness*
// (tests/host_harness), the same phases run as `for (lane = 0..63)` loops, which lets the
// CPU-only test tier execute the exact wave algorithm (index maths, carries, block-parallel
// timing recovery) against the oracle without a GPU.  The shipped library contains only the
// gfx950 build; there is no CPU fallback in the product.
//
// THE SEAM.  Everything that differs between the two builds lives in this header and in wave_ops.hpp beside it (the
// float-vector, LDS and DPP primitives), under ONE predicate, DH_ON_GPU.  Every primitive states once what it computes
// (NaN behaviour and which lanes' results are defined included), has its gfx950 form and its CPU restatement side by side,
// and carries the same name and signature in both builds.  The algorithm bodies (*_core.hpp) are a single program: new code
// never writes a build conditional inside a body -- it adds a primitive here.  The only build conditionals outside the two
// headers are whole-function pairs at namespace scope, a hand-scheduled kernel piece next to its plain restatement
// (dh_fir_lane, dh_fir_mfma, dh_fir_f16, dh_agc_scan, the Viterbi forward passes); what the CPU tier proves about the device
// code it proves through the agreement of these pairs.  tests/test_device_seam.py keeps the rule from eroding.
#pragma once

#include <stdint.h>
#include <stddef.h>

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define DH_DEVICE_BUILD 1
#define DH_HD __host__ __device__ __forceinline__
#define DH_D __device__ __forceinline__
#else
#define DH_DEVICE_BUILD 0
#define DH_HD inline
#define DH_D inline
#endif

// the device pass of the gfx950 build: the one predicate of the seam (0 in the CPU harness and in hipcc's host pass)
#if DH_DEVICE_BUILD && defined(__HIP_DEVICE_COMPILE__)
#define DH_ON_GPU 1
#else
#define DH_ON_GPU 0
#endif

// an expression that differs between the builds, both forms side by side
#if DH_ON_GPU
#define DH_GPU_ELSE(gpu, cpu) gpu
#else
#define DH_GPU_ELSE(gpu, cpu) cpu
#endif

#define DH_WAVE 64

#if DH_ON_GPU
// DH_FOR_LANES_FRESH: the lane id passes through an empty volatile asm, so nothing derived from it (per-lane LDS
// addresses, lane % 10, 64-bit row pointers) is loop-invariant to the compiler.  Left alone it hoists dozens of such
// values out of the slicer's per-run loop, across the FIR where every register is taken, spills them to scratch and
// reloads them with dependent memory round trips inside the latency-bound phases; recomputing them costs a few VALU
// instructions per phase instead.  Used for the phases inside that loop; everything else uses DH_FOR_LANES.
static __device__ __forceinline__ int dh_fresh_lane_id_() { int l = (int) threadIdx.x; asm volatile("" : "+v"(l)); return l; }
#define DH_FOR_LANES(lane) for (int lane = (int) threadIdx.x, dh_once_ = 1; dh_once_; dh_once_ = 0)
#define DH_FOR_LANES_FRESH(lane) for (int lane = dh_fresh_lane_id_(), dh_once_ = 1; dh_once_; dh_once_ = 0)
// The phases of a body exchange data through LDS only, so the barrier orders LDS traffic only: __syncthreads() also fences
// GLOBAL memory, which makes the compiler wait (s_waitcnt vmcnt(0)) for every global load in flight -- the next window's
// loads, requested a phase earlier precisely so that they can stay in flight through the phases that follow (round 3: the wait
// sat in front of the slicing phase and cost 1 ms of a 6.8 ms step).  Where a body hands data to another one through global
// memory the caller fences explicitly (chain_core.hpp: dh_barrier_global() between slicer and decoder, workgroup scope).
#define DH_BARRIER() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local"); __builtin_amdgcn_s_barrier(); \
                          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local"); } while (0)
#define DH_BALLOT_ACC(mask, pred, lane) (mask) = __builtin_amdgcn_ballot_w64((bool) (pred))      /* (v_cmp straight into the scalar pair; __ballot((pred) ? 1 : 0) left a v_cndmask + v_cmp behind every vote) */
#else
#define DH_FOR_LANES(lane) for (int lane = 0; lane < DH_WAVE; ++lane)
#define DH_FOR_LANES_FRESH(lane) DH_FOR_LANES(lane)
#define DH_BARRIER() ((void) 0)
#define DH_BALLOT_ACC(mask, pred, lane) (mask) |= ((uint64_t) ((pred) ? 1 : 0) << (lane))
#endif
#define DH_IS_LANE0(lane) ((lane) == 0)
// DH_IS_LANE0 outside a lane loop: true in the ONE lane that performs a body's wave-uniform global stores (the CPU build runs
// such code once, for all lanes)
DH_HD bool dh_is_writer_lane() { return DH_GPU_ELSE(threadIdx.x == 0, true); }

// A value every lane holds identically (loaded from LDS / memory at a wave-uniform address): moving it to a
// scalar register lets the arithmetic that follows run on the scalar ALU instead of costing VALU issue cycles.
DH_HD uint32_t dh_uniform(uint32_t x) { return DH_GPU_ELSE((uint32_t) __builtin_amdgcn_readfirstlane((int) x), x); }

// ---------------------------------------------------------------------------------------------
// A word in global memory that workgroups of ONE launch hand a channel over through (chain_core.hpp: the flag word of the tail
// split).  Nothing here orders anything by itself: the word is read and merged relaxed, at agent scope, and the two fences
// stand on either side of it.  The CPU build runs the workgroups of a launch one after the other, in index order, in one
// thread: every access is a plain one, a fence is nothing.
//   dh_agent_load(p)              the word
//   dh_agent_cas(p, seen, want)   stores `want` if the word is still `seen` (true); otherwise `seen` becomes what it holds now
//   dh_agent_add(p, v)            adds v to the word (a statistic: nobody waits for it)
//   dh_nap()                      between two looks at a word that another workgroup will store (s_sleep 64: ~2 us)
//   dh_acquire_behind_flag()      after the word was seen: nothing older than it stays in this CU's L1 (buffer_inv) or scalar cache
//   dh_release_before_flag()      in front of the store of the word: everything this workgroup stored has reached the XCD's L2
//                                 (s_waitcnt, no write-back: the workgroup that reads the word runs on the same XCD)
//   dh_xcc_id()                   the XCD this wavefront runs on (HW_REG_XCC_ID; the CPU build: 0)
//   dh_opaque_scalar(x)           x, as a scalar the compiler cannot tie to an earlier computation of the same value
//   dh_barrier_global()           the workgroup's barrier that also fences GLOBAL memory at workgroup scope (__syncthreads; DH_BARRIER
//                                 orders LDS only): one body's global stores, read back by the body behind it in the same wavefront
DH_HD uint32_t dh_agent_load(const uint32_t* p) { return DH_GPU_ELSE(__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), *p); }
DH_HD bool dh_agent_cas(uint32_t* p, uint32_t& seen, uint32_t want) {
#if DH_ON_GPU
    return __hip_atomic_compare_exchange_strong(p, &seen, want, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    if (*p == seen) { *p = want; return true; }
    seen = *p;
    return false;
#endif
}
DH_HD void dh_agent_add(uint32_t* p, uint32_t v) { DH_GPU_ELSE(__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), *p += v); }
DH_HD uint32_t dh_xcc_id() { return DH_GPU_ELSE(__builtin_amdgcn_s_getreg((31 << 11) | 20) & 15u, 0u); }
#if DH_ON_GPU
__device__ __forceinline__ void dh_nap() { __builtin_amdgcn_s_sleep(64); }
__device__ __forceinline__ void dh_acquire_behind_flag() { __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent"); __builtin_amdgcn_s_dcache_inv(); }
__device__ __forceinline__ void dh_release_before_flag() { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); }
__device__ __forceinline__ uint32_t dh_opaque_scalar(uint32_t x) { asm volatile("" : "+s"(x)); return x; }
__device__ __forceinline__ void dh_barrier_global() { __syncthreads(); }
#else
inline void dh_nap() {}
inline void dh_acquire_behind_flag() {}
inline void dh_release_before_flag() {}
inline uint32_t dh_opaque_scalar(uint32_t x) { return x; }
inline void dh_barrier_global() {}
#endif

DH_HD int dh_popc32(uint32_t x) { return DH_GPU_ELSE(__popc(x), __builtin_popcount(x)); }
DH_HD int dh_popc64(uint64_t x) { return DH_GPU_ELSE(__popcll(x), __builtin_popcountll(x)); }
DH_HD int dh_ffs64(uint64_t x) { return DH_GPU_ELSE(__ffsll((unsigned long long) x) - 1, __builtin_ctzll(x)); }      // index of the lowest set bit, x != 0
DH_HD int dh_top64(uint64_t x) { return 63 - DH_GPU_ELSE(__clzll((long long) x), __builtin_clzll(x)); }              // index of the highest set bit, x != 0

DH_HD uint32_t dh_brev32(uint32_t x) {
#if DH_ON_GPU
    return __brev(x);
#else
    x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
    x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
    x = ((x >> 4) & 0x0F0F0F0Fu) | ((x & 0x0F0F0F0Fu) << 4);
    x = ((x >> 8) & 0x00FF00FFu) | ((x & 0x00FF00FFu) << 8);
    return (x >> 16) | (x << 16);
#endif
}

// ---------------------------------------------------------------------------------------------
// The launch vocabulary of the helper kernels (at the end of the core header that owns their bodies; helper_launches.hpp for
// the batch FEC and stand-alone stages): their __global__ wrappers and launch statements are one text for both builds.  A
// launcher ends in dh_launch(kernel, grid, block, lds_bytes, stream, what, args...), 0 = launched.  hipcc gives the words their usual meaning (in its host pass too, hence DH_DEVICE_BUILD here); in the
// CPU build __global__ is a plain function, blockIdx / threadIdx / blockDim / gridDim are thread-local (tests push from several
// host threads), __shared__ is storage that outlives the call, the atomics on the monitor's summary words are plain updates,
// and dh_launch is a loop: the kernel called once per (block, thread) of the grid the launcher computed, LAST FIRST --
// the lanes of a launch have no order, and nothing may come to rest on one.
//   dh_workgroup(lanes)   the block of a kernel whose body runs its own lane loops (DH_FOR_LANES, DH_OP_FOR): dim3(lanes) on
//                         the device; the CPU build visits such a block once
#if DH_DEVICE_BUILD
static inline dim3 dh_workgroup(unsigned lanes) { return dim3(lanes); }
// (engine.hip defines it: hipLaunchKernelGGL, then the one launch-failure check, whose message is `what`)
template <class K, class... A>
static int dh_launch(K kernel, dim3 grid, dim3 block, size_t lds_bytes, void* stream, const char* what, const A&... args);
#else
struct dim3 {
    unsigned x, y, z; bool lanes_in_body = false;
    dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {}
};
static inline dim3 dh_workgroup(unsigned lanes) { dim3 d(lanes); d.lanes_in_body = true; return d; }
struct DhLaunchIndex { unsigned x, y, z; };
inline thread_local DhLaunchIndex blockIdx, threadIdx, blockDim, gridDim;
#define __global__ static
#define __launch_bounds__(...)
#define __shared__ static thread_local
template <class T> inline T atomicAdd(T* p, T v) { const T old = *p; *p = old + v; return old; }
template <class T> inline T atomicMin(T* p, T v) { const T old = *p; if (v < old) *p = v; return old; }
template <class K, class... A>
inline int dh_launch(K kernel, dim3 grid, dim3 block, size_t /* lds_bytes */, void* /* stream */, const char* /* what */, const A&... args) {
    const dim3 threads = block.lanes_in_body ? dim3(1) : block;
    gridDim = { grid.x, grid.y, grid.z }; blockDim = { block.x, block.y, block.z };
    for (unsigned bz = grid.z; bz-- > 0;) for (unsigned by = grid.y; by-- > 0;) for (unsigned bx = grid.x; bx-- > 0;)
        for (unsigned tz = threads.z; tz-- > 0;) for (unsigned ty = threads.y; ty-- > 0;) for (unsigned tx = threads.x; tx-- > 0;) {
            blockIdx = { bx, by, bz }; threadIdx = { tx, ty, tz };
            kernel(args...);
        }
    return 0;
}
#endif
// the stream of a back end; a back end without one (the stand-alone test programs') launches on the null stream
template <class BE> static auto dh_be_stream(BE& be, int) -> decltype((void*) be.ms()) { return (void*) be.ms(); }
template <class BE> static void* dh_be_stream(BE&, long) { return nullptr; }
// the grid of a one-item-per-lane kernel with a grid-stride loop
inline unsigned grid_for(size_t n, unsigned block) {
    const size_t g = (n + block - 1) / block;
    return (unsigned) (g < 1 ? 1 : (g > 8192 ? 8192 : g));      // 256 CUs x 32 resident workgroups, grid-stride beyond
}

template <typename T> DH_HD T dh_min(T a, T b) { return a < b ? a : b; }
template <typename T> DH_HD T dh_max(T a, T b) { return a > b ? a : b; }

// branch weights: what the register allocator keeps out of the hot path (spill code goes where the weights are low)
#define DH_LIKELY(x) __builtin_expect(!!(x), 1)
#define DH_UNLIKELY(x) __builtin_expect(!!(x), 0)

// DH_TO_VGPR: a loop-invariant wave-uniform value that should live in a VGPR rather than compete for the 102 SGPRs
// DH_COMPILER_FENCE: compiler-only memory fence -- values cached from memory before it must be re-read after it
// (the CPU build: nothing, both)
// DH_CONST_TABLE: a constant table both builds index at run time -- on the device it needs an address in device memory
#if DH_ON_GPU
#define DH_TO_VGPR(x) asm volatile("" : "+v"(x))
#define DH_COMPILER_FENCE() asm volatile("" ::: "memory")
#define DH_CONST_TABLE __device__ static constexpr
#else
#define DH_TO_VGPR(x) ((void) 0)
#define DH_COMPILER_FENCE() ((void) 0)
#define DH_CONST_TABLE static constexpr
#endif

// Markers: with -DDH_ASM_MARKERS (tools/asm_census.py) every phase boundary of the slicer (DH_PHASE_MARK*) and every region
// of the decoders (DH_DMARK) leaves a comment in the assembly, which the census counts instructions between; nothing otherwise.
// (Round 2-4's per-phase shader-clock builds used the same places; they went with round 5's prune.)
#if defined(DH_ASM_MARKERS) && DH_ON_GPU
#define DH_PHASE_MARK_BEGIN() asm volatile("; DH_PHASE begin" ::: "memory")
#define DH_PHASE_MARK(i) asm volatile("; DH_PHASE " #i ::: "memory")
#define DH_DMARK(text) asm volatile("; DH_DMARK " text ::: "memory")
#else
#define DH_PHASE_MARK_BEGIN() ((void) 0)
#define DH_PHASE_MARK(i) ((void) 0)
#define DH_DMARK(text) ((void) 0)
#endif

// ---------------------------------------------------------------------------------------------
// Values a lane holds across phases: registers on the GPU, [lane] arrays in the CPU build.
//   DH_LANE_ARRAY(type, name, n) / DH_LA(name, lane)      n values per lane; DH_LA(name, lane)[i] is this lane's i-th
//   DH_LANE_VALUE(type, name) / DH_LV(name, lane)         one value per lane
//     DH_LV_READ(name, k)        the value of lane k, k wave-uniform (v_readlane)
//     DH_LV_DOWN(name, lane, d)  the value of lane + d; the lane's own where lane + d > 63 (__shfl_down)
//   DH_LANE_STRUCT(type, name) / DH_LS(name, lane)        a struct of 32-bit fields per lane; as a parameter: DH_LANE_STRUCT_REF, and
//                                                          DH_LANE_STRUCT_IN for one only read (the device passes it by value)
//     DH_LS_READ(name, field, k)      field of lane k, k wave-uniform (v_readlane)
//     DH_LS_WRITE(name, field, k, v)  sets it, k and v wave-uniform (v_writelane: dh_writelane)
//     DH_LS_GATHER(name, field, j)    field of lane j, j a per-lane value (ds_bpermute; every lane of the wave takes part)
//   DH_LANES_BELOW(mask, lane)   the number of set bits of `mask` below this lane: an exclusive prefix count of a vote (v_mbcnt)
#if DH_ON_GPU
#define DH_LANE_ARRAY(type, name, n) type name[n]
#define DH_LA(name, lane) name
#define DH_LANE_VALUE(type, name) type name
#define DH_LV(name, lane) name
#define DH_LV_READ(name, k) ((uint32_t) __builtin_amdgcn_readlane((int) (name), (int) (k)))
#define DH_LV_DOWN(name, lane, d) ((uint32_t) __shfl_down((int) (name), (unsigned) (d), DH_WAVE))
#define DH_LANE_STRUCT(type, name) type name
#define DH_LANE_STRUCT_REF(type, name) type& name
#define DH_LANE_STRUCT_IN(type, name) const type name
#define DH_LS(name, lane) name
#define DH_LS_READ(name, field, k) ((uint32_t) __builtin_amdgcn_readlane((int) (name).field, (int) (k)))
// (v_writelane takes value and lane from scalar registers, a VOP3 of gfx9 reads at most one: the lane select goes through m0,
// which belongs to the compiler -- a clobber would be ignored -- hence saved and restored around the write)
static __device__ __forceinline__ uint32_t dh_writelane(uint32_t reg, uint32_t lane, uint32_t v) {
    const uint32_t sv = (uint32_t) __builtin_amdgcn_readfirstlane((int) v), si = (uint32_t) __builtin_amdgcn_readfirstlane((int) lane);
    uint32_t keep;
    asm("s_mov_b32 %1, m0\n\ts_mov_b32 m0, %3\n\tv_writelane_b32 %0, %2, m0\n\ts_mov_b32 m0, %1" : "+v"(reg), "=&s"(keep) : "s"(sv), "s"(si));
    return reg;
}
#define DH_LS_WRITE(name, field, k, v) (name).field = dh_writelane((name).field, (uint32_t) (k), (uint32_t) (v))
#define DH_LS_GATHER(name, field, j) ((uint32_t) __shfl((int) (name).field, (int) (j), DH_WAVE))
#define DH_LANES_BELOW(mask, lane) ((uint32_t) __builtin_amdgcn_mbcnt_hi((uint32_t) ((mask) >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) (mask), 0u)))
#else
#define DH_LANE_ARRAY(type, name, n) type name[DH_WAVE][n]
#define DH_LA(name, lane) name[lane]
#define DH_LANE_VALUE(type, name) type name[DH_WAVE]
#define DH_LV(name, lane) name[lane]
#define DH_LV_READ(name, k) ((uint32_t) name[k])
#define DH_LV_DOWN(name, lane, d) ((uint32_t) name[((lane) + (d)) < DH_WAVE ? (lane) + (d) : (lane)])
#define DH_LANE_STRUCT(type, name) type name[DH_WAVE]
#define DH_LANE_STRUCT_REF(type, name) type* name
#define DH_LANE_STRUCT_IN(type, name) const type* name
#define DH_LS(name, lane) name[lane]
#define DH_LS_READ(name, field, k) ((uint32_t) (name)[k].field)
#define DH_LS_WRITE(name, field, k, v) (name)[k].field = (uint32_t) (v)
#define DH_LS_GATHER(name, field, j) ((uint32_t) (name)[j].field)
#define DH_LANES_BELOW(mask, lane) ((uint32_t) dh_popc64((mask) & (((uint64_t) 1 << (lane)) - 1u)))
#endif

// DH_WAVE words of a wavefront in ONE vector register, word i in lane i, indexed with run-time (wave-uniform) indices:
// v_readlane / v_writelane take the index from a scalar register, so a read or write is a single instruction with no memory
// round trip (an LDS copy costs ~100 cycles of latency per access on a serial path, a register array would go to scratch).
// s[i] reads, s[i] = v writes; load / store move all of them, store_words the words [first, first + n).  The CPU build is a
// plain array.  (DhState: the decoders' channel state, decoder_core.hpp, is what it holds.)
struct DhState {
#if DH_ON_GPU
    uint32_t reg;
    __device__ __forceinline__ uint32_t get(uint32_t i) const { return (uint32_t) __builtin_amdgcn_readlane((int) reg, (int) i); }
    __device__ __forceinline__ void set(uint32_t i, uint32_t v) { reg = dh_writelane(reg, i, v); }
    __device__ __forceinline__ void load(const uint32_t* g) { reg = threadIdx.x < DH_WAVE ? g[threadIdx.x] : 0u; }
    __device__ __forceinline__ void store(uint32_t* g) const { if (threadIdx.x < DH_WAVE) g[threadIdx.x] = reg; }
    __device__ __forceinline__ void store_words(uint32_t* g, uint32_t first, uint32_t n) const { if (threadIdx.x - first < n) g[threadIdx.x - first] = reg; }
#else
    uint32_t w[DH_WAVE];
    uint32_t get(uint32_t i) const { return w[i]; }
    void set(uint32_t i, uint32_t v) { w[i] = v; }
    void load(const uint32_t* g) { for (int i = 0; i < DH_WAVE; i++) w[i] = g[i]; }
    void store(uint32_t* g) const { for (int i = 0; i < DH_WAVE; i++) g[i] = w[i]; }
    void store_words(uint32_t* g, uint32_t first, uint32_t n) const { for (uint32_t i = 0; i < n; i++) g[i] = w[first + i]; }
#endif
    struct Ref {
        DhState* st; uint32_t i;
        DH_HD operator uint32_t() const { return st->get(i); }
        DH_HD Ref& operator=(uint32_t v) { st->set(i, v); return *this; }
        DH_HD Ref& operator=(const Ref& o) { st->set(i, (uint32_t) o); return *this; }
        DH_HD uint32_t operator++(int) { const uint32_t v = st->get(i); st->set(i, v + 1u); return v; }
    };
    DH_HD Ref operator[](uint32_t i) { return Ref{this, i}; }
    DH_HD Ref operator[](int i) { return Ref{this, (uint32_t) i}; }
};

// ---------------------------------------------------------------------------------------------
// The same vocabulary for a workgroup of DH_OP_LANES lanes = DH_OP_WAVES wavefronts whose phases span the whole workgroup (the
// scan of the packed read-out, outpack_core.hpp): the CPU build's lane loop runs over all 256 lanes, a per-lane value is an
// array of 256, a per-wavefront value (a vote: a scalar pair on the device) an array of four.
//   DH_OP_FOR(lane)                                    the lane loop
//   DH_OP_VAL(type, name) / DH_OP_V(name, lane)        a value per lane: a register
//   DH_OP_WAVE_VAL(type, name) / DH_OP_W(name, lane)   a value per wavefront, as the lane's wavefront holds it: a scalar pair
//   DH_OP_VOTE(name, pred, lane)     the wavefront's vote on pred, bit l = its lane l; DH_OP_CLEAR_VOTES(name) before the loop that votes
//   DH_OP_WAVE_SCAN(name)            inclusive prefix sum inside each wavefront (64-bit values): six steps of "add what the lane d
//                                    below holds" (ds_bpermute)
//   DH_OP_WAVE_MAX(dst, src)         the largest value (unsigned, 32 bits) of each wavefront, in all of its lanes
#define DH_OP_LANES 256u                    /* lanes of the scan's workgroup = channels one pass of the scan covers */
#define DH_OP_WAVES (DH_OP_LANES / DH_WAVE)
#if DH_ON_GPU
#define DH_OP_FOR(lane) for (uint32_t lane = threadIdx.x, dh_once_ = 1; dh_once_; dh_once_ = 0)
#define DH_OP_VAL(type, name) type name[1]
#define DH_OP_WAVE_VAL(type, name) type name[1]
#define DH_OP_V(name, lane) name[0]
#define DH_OP_W(name, lane) name[0]
#define DH_OP_VOTE(name, pred, lane) name[0] = __builtin_amdgcn_ballot_w64((bool) (pred))
#define DH_OP_CLEAR_VOTES(name) ((void) 0)
#define DH_OP_WAVE_SCAN(name) do { \
        const uint32_t wl_ = threadIdx.x & (DH_WAVE - 1u); \
        for (uint32_t d_ = 1; d_ < DH_WAVE; d_ <<= 1) { \
            const uint64_t t_ = (uint64_t) __shfl_up((unsigned long long) name[0], d_, DH_WAVE); \
            if (wl_ >= d_) name[0] += t_; \
        } } while (0)
#define DH_OP_WAVE_MAX(dst, src) do { \
        dst[0] = src[0]; \
        for (uint32_t d_ = 1; d_ < DH_WAVE; d_ <<= 1) { const uint32_t t_ = (uint32_t) __shfl_xor((int) dst[0], (int) d_, DH_WAVE); if (t_ > dst[0]) dst[0] = t_; } \
    } while (0)
#else
#define DH_OP_FOR(lane) for (uint32_t lane = 0; lane < DH_OP_LANES; ++lane)
#define DH_OP_VAL(type, name) type name[DH_OP_LANES]
#define DH_OP_WAVE_VAL(type, name) type name[DH_OP_WAVES]
#define DH_OP_V(name, lane) name[lane]
#define DH_OP_W(name, lane) name[(lane) / DH_WAVE]
#define DH_OP_VOTE(name, pred, lane) name[(lane) / DH_WAVE] |= (uint64_t) ((pred) ? 1 : 0) << ((lane) % DH_WAVE)
#define DH_OP_CLEAR_VOTES(name) do { for (uint32_t w_ = 0; w_ < DH_OP_WAVES; ++w_) name[w_] = 0; } while (0)
#define DH_OP_WAVE_SCAN(name) do { for (uint32_t l_ = 1; l_ < DH_OP_LANES; ++l_) if (l_ % DH_WAVE) name[l_] += name[l_ - 1]; } while (0)
#define DH_OP_WAVE_MAX(dst, src) do { \
        for (uint32_t w_ = 0; w_ < DH_OP_WAVES; ++w_) { \
            uint32_t m_ = 0; \
            for (uint32_t l_ = 0; l_ < DH_WAVE; ++l_) if (src[w_ * DH_WAVE + l_] > m_) m_ = src[w_ * DH_WAVE + l_]; \
            for (uint32_t l_ = 0; l_ < DH_WAVE; ++l_) dst[w_ * DH_WAVE + l_] = m_; \
        } } while (0)
#endif
