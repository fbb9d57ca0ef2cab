// Shared device helpers for the lc_amd HIP kernels (gfx950 / CDNA4, wave64).  The fp64 cross-lane layer (DPP / permlane exchanges,
// wave_allreduce, wave_reduce_scatter16, tri6) lives in shared/lc_shared.h, which the pose-covariance library includes as well.
#pragma once
#include <hip/hip_runtime.h>

#include "shared/lc_shared.h"

namespace lc {

// 16-byte store of a write-once stream (a gradient map the kernel never re-reads): non-temporal, so that it does not push the
// maps the next kernel re-reads out of L2 / Infinity Cache (measured on the keypoint head: profiles/r02/head_policy.txt).
typedef float lc_v4f_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void store_stream4(float* q, float a, float b, float c, float d) {
    lc_v4f_t r = {a, b, c, d};
    __builtin_nontemporal_store(r, reinterpret_cast<lc_v4f_t*>(q));
}


// 1/x without the IEEE division sequence: v_rcp_f64 (measured 4.5e-8 relative on gfx950, scripts/ubench/rcp_accuracy.cpp)
// + one Newton step -> 2.2e-15.  x finite, non-zero, normal -- every use is a pivot, a depth or a norm that is checked
// separately.  ~29 cycles for a lone wave against ~72 for `1.0 / x` (scripts/ubench/fp64_latency.cpp).
__device__ __forceinline__ double fast_rcp(double x) {
    const double y = __builtin_amdgcn_rcp(x);
    const double e = __builtin_fma(-x, y, 1.0);
    return __builtin_fma(y, e, y);
}

// sqrt(x) and 1/sqrt(x) from v_rsq_f64 + one coupled Goldschmidt step (4e-15 relative; ~39 cycles against ~104 for sqrt()).
// x >= 0; x == 0 gives sqrt 0 / rsqrt +inf.
__device__ __forceinline__ void fast_sqrt_rsqrt(double x, double& s, double& rs) {
    const double r0 = __builtin_amdgcn_rsq(x);
    const double g = x * r0, h = 0.5 * r0;
    const double rr = __builtin_fma(-h, g, 0.5);
    const double g1 = __builtin_fma(g, rr, g), h1 = __builtin_fma(h, rr, h);
    s = x == 0.0 ? 0.0 : g1;
    rs = x == 0.0 ? r0 : 2.0 * h1;
}
__device__ __forceinline__ double fast_sqrt(double x) {
    double s, rs;
    fast_sqrt_rsqrt(x, s, rs);
    return s;
}

// The same for x > 0 only (the caller has tested it): the arithmetic of fast_sqrt_rsqrt without its compare and its two 64-bit selects
// for x == 0 -- the same bits wherever x > 0.
__device__ __forceinline__ void fast_sqrt_rsqrt_pos(double x, double& s, double& rs) {
    const double r0 = __builtin_amdgcn_rsq(x);
    const double g = x * r0, h = 0.5 * r0;
    const double rr = __builtin_fma(-h, g, 0.5);
    s = __builtin_fma(g, rr, g);
    rs = 2.0 * __builtin_fma(h, rr, h);
}

// Ordering point between the lanes of ONE wavefront that hand data to each other through LDS.  The wave barrier alone is a
// scheduling barrier (IntrNoMem); the wavefront-scope release / acquire pair around it makes the hand-off part of the memory
// model -- the compiler may not move a lane's ds_read above another lane's ds_write across it -- and emits no instruction on
// gfx950 (a wave's DS operations execute in order; checked: identical instruction counts in the ISA with and without the pair).
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Sum of K doubles per lane over the 64 lanes of a ONE-wavefront workgroup, result in every lane, through LDS.
// Lane t stores v[k] at lds[k*68 + t + 2*(t/32)] (32-double segments padded by 16 bytes, rows of 68 doubles: conflict-free
// ds_write_b64 and ds_read_b128); lane r < 2 K sums one segment with eight + eight 16-byte reads, the two partial sums of a row meet
// by DPP, the K totals are re-read by all lanes.  Measured cheaper than the permlane/DPP reduce-scatter + broadcast for a lone wave WITH
// ALL 28 ENTRIES (a reduce-scatter of 32: 30 exchanges; a dependent 64-bit cross-lane exchange costs 25-32 cycles,
// scripts/ubench/fp64_latency.cpp).  That measurement does not carry over to the 14 entries a wave of the two-wave team owns: there the
// register tree (16 exchanges of 7 instructions or fewer, block_sum_team2_reg below) is the faster form -- the sum itself is ~100 cycles
// longer than through LDS, the per-point phase ~230 cycles shorter without its 14 stores (profiles/teamreg/NOTES.md).  The one-wave form
// with 14 + 14 entries in registers has not been measured.  Needs K <= 32 and K*68 + K doubles of LDS.
// (Four-wave workgroups sum in registers too: block_sum_waves4 below.)
// The sum is called in two halves: block_sum_open() (the previous totals have been read), then the caller stores its K values itself
// with block_sum_put() AS IT PRODUCES THEM -- the LDS stores of a lone wave drain at about 40 B/clk (MI355X_MICROARCH.md, LDS: one wave
// gets half the store rate), 360 cycles for 28 doubles x 64 lanes, and issued early they drain behind the arithmetic that produces
// the later values -- then block_sum_close() for the reduction and the broadcast.
// The ordering points of the LDS hand-offs inside the sum are wave_sync(): a workgroup of ONE wavefront needs no barrier and no
// drain -- the DS operations of a wave execute in program order (a ds_read issued after a ds_write of another lane's slot returns the
// new value), so the reads simply queue behind the stores and the wave stalls only where it consumes a loaded value; a
// __syncthreads() there costs an `s_waitcnt lgkmcnt(0)` -- a full drain of the LDS queue -- three times per sum (measured with
// scripts/ubench/pnp_ab.py).
constexpr int block_sum_lds_doubles(int K) { return K * 68 + K; }
__device__ __forceinline__ int block_sum_open(int lane) {
    wave_sync();  // the previous totals have been read
    return lane + 2 * (lane >> 5);
}
template <int ROW = 68>  // doubles between the rows of two entries (the team form has its own, kTeamRowDoubles below)
__device__ __forceinline__ void block_sum_put(double* lds, int pos, int k, double v) { lds[k * ROW + pos] = v; }

// sum of one 32-double segment of a row (sixteen 16-byte reads): the order every form of the LDS block sum adds a segment in
__device__ __forceinline__ double block_sum_segment(const double2* row) {
    double2 a[8];  // two batches of eight 16-byte reads: keeps the register peak (and so the occupancy) down
#pragma unroll
    for (int i = 0; i < 8; ++i) a[i] = row[i];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const double2 t = row[8 + i];
        a[i].x += t.x;
        a[i].y += t.y;
    }
#pragma unroll
    for (int st = 4; st >= 1; st >>= 1) {
#pragma unroll
        for (int i = 0; i < st; ++i) { a[i].x += a[i + st].x; a[i].y += a[i + st].y; }
    }
    return a[0].x + a[0].y;
}
// One COMPONENT of that tree, for a segment dealt to two lanes: block_sum_segment adds the 32 doubles d[0..31] of a segment as
// d[j] + d[j + 16], then + 8, + 4, + 2 (a[i] += a[i + st] on 16-byte pairs), and only its last add, d[0] + d[1], joins an even-indexed
// double (.x of a pair) with an odd-indexed one (.y).  This is everything before that add for the 16 doubles of one parity -- `d` points at
// the segment's double 0 (.x) or 1 (.y) -- in the same order; the caller's x + y is block_sum_segment's total bit for bit.
__device__ __forceinline__ double block_sum_segment_component(const double* d) {
    double a[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) a[i] = d[2 * i];
#pragma unroll
    for (int i = 0; i < 8; ++i) a[i] += d[16 + 2 * i];
#pragma unroll
    for (int st = 4; st >= 1; st >>= 1) {
#pragma unroll
        for (int i = 0; i < st; ++i) a[i] += a[i + st];
    }
    return a[0];
}

template <int K>
__device__ __forceinline__ void block_sum_close(double (&v)[K], double* lds, int lane) {
    static_assert(K <= 32, "two segments per entry, one lane each");
    wave_sync();
    double s = 0;
    if (lane < 2 * K) s = block_sum_segment(reinterpret_cast<const double2*>(lds + (lane / 2) * 68 + 34 * (lane % 2)));
    s += dpp_mov_f64<kDppQuadXor1>(s, s);
    double* tot = lds + K * 68;
    if (lane < 2 * K && (lane % 2) == 0) tot[lane / 2] = s;
    wave_sync();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = tot[k];
}

// Values handed from one workgroup to another INSIDE a launch (the workgroups may sit on different XCDs, whose L2s are not
// coherent with each other): written through and read around the caches as agent-scope relaxed atomics (sc1 accesses).  The
// writer orders them before its arrival count with xcd_stores_done() + a workgroup barrier; no cache-wide fence anywhere
// (profiles/r03/NOTES.md 4.1 "Tiled form" has the measurements behind this choice).
template <class T>
__device__ __forceinline__ void xcd_store(T* q, T v) { __hip_atomic_store(q, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <class T>
__device__ __forceinline__ T xcd_load(const T* q) { return __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void xcd_stores_done() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// "Which workgroup finishes last" for grids of hundreds of workgroups that all finish together: arrivals on ONE word are served one
// after the other (11-13 ns each: 512 of them are 6 us behind a 10 us kernel), so the workgroups count themselves in on one of
// kArrivalShards words, each on a 128-byte line of its own (neighbours in dispatch order -> different words), and only the last of a
// shard goes on to the top word.  `words`: kArrivalWords zeroed unsigned, left zeroed by arrival_reset() (called by the workgroup
// that got `true`, after its last use of what the others wrote).  Called by ONE thread, after xcd_stores_done().
constexpr int kArrivalShards = 16, kArrivalStride = 32;
constexpr int kArrivalWords = (1 + kArrivalShards) * kArrivalStride;
__device__ __forceinline__ bool arrive_is_last(unsigned* words, unsigned block, unsigned blocks) {
    const unsigned shards = blocks < (unsigned)kArrivalShards ? blocks : (unsigned)kArrivalShards;
    const unsigned g = block % shards, members = (blocks - g + shards - 1) / shards;
    if (__hip_atomic_fetch_add(words + (1 + g) * kArrivalStride, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != members - 1) return false;
    return __hip_atomic_fetch_add(words, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == shards - 1;
}
__device__ __forceinline__ void arrival_reset(unsigned* words, int tid) {
    if (tid <= kArrivalShards) xcd_store(words + tid * kArrivalStride, 0u);
}

// (The LDS form of the team's sum: built with -DLC_PNP_TEAM_REGSUM=0; the shipped form is block_sum_team2_reg below.)
// The one-wave sum played by a TEAM of two wavefronts that both hold all 64 values of every entry (lane = point in both:
// the pose unit's latency build, where half the SIMDs idle next to a wave that is bound by instruction issue).  Wave W produces and
// stores only the entries k with k % 2 == W -- block_sum_put<kTeamRowDoubles>, the slots of the one-wave form in rows of the team's own
// stride -- and sums them itself on 2 K lanes: lane l takes component l % 2 (.x / .y of the 16-byte pairs) of segment (l / 2) % 2 of
// entry 2 (l / 4) + W, 15 adds where a lane with a whole segment issues 31 (a VALU instruction costs the same for any number of active
// lanes).  One quad exchange joins the components -- block_sum_segment's last add, a[0].x + a[0].y -- and a second one the two
// segments, as block_sum_close<K> joins them: every total has the one-wave form's bits.
// LDS banks: the component reads are 8-byte reads of stride 16 bytes (the compiler pairs them into ds_read2_b64: banks (a / 4) % 32,
// groups of 16 consecutive lanes, i.e. four entries; a lone ds_read_b64: % 64, 32 lanes, eight entries).  The four lanes of an entry start
// 0, 2, 4 and 6 dwords into its row (34 doubles between the segments = 4 dwords mod 64) and cover 8 consecutive banks, so the rows of
// consecutive entries OF ONE WAVE, 2 kTeamRowDoubles doubles apart, must start an odd multiple of 8 dwords apart: kTeamRowDoubles = 2,
// 6, 10 or 14 mod 16.  66 is the smallest that holds the 32 + 2 + 32 doubles of a row; the one-wave form's 68 puts entries q and q + 2 of
// a group on the same banks (2-way; measured: profiles/teamsum/NOTES.md).  The stores (lane t at t + 2 (t / 32), 16 lanes = 32
// consecutive dwords) are conflict-free at any row stride.
// A wave's rows are written and read by that wave alone (DS operations of a wave execute in program order: no
// barrier between its stores and its reads); the K / 2 totals of each wave meet in one of TWO rows of totals behind the slots, then
// ONE workgroup barrier, then every thread of both waves reads all K.  The rows alternate by `phase` (toggled by the call, as in
// block_sum_waves4): a wave still reading the totals of sum e is not overwritten by sum e + 1, and whoever writes sum e + 2 has
// passed the barrier of e + 1, which the other wave only reaches with its reads of e done.  lds: sum_team2_lds_doubles(K) doubles.
constexpr int kTeamRowDoubles = 66;
static_assert(kTeamRowDoubles >= 66 && kTeamRowDoubles % 4 == 2, "a row holds two padded segments; rows of one wave fall on different banks");
constexpr int sum_team2_lds_doubles(int K) { return K * kTeamRowDoubles + 2 * K; }
template <int K, int W>
__device__ __forceinline__ void block_sum_team2(double (&v)[K], double* lds, int lane, int& phase) {
    static_assert(K % 2 == 0 && K <= 32 && (W == 0 || W == 1), "an even number of entries dealt to two waves");
    wave_sync();  // this wave's stores are in its LDS queue
    double s = 0;
    const int comp = lane & 1, seg = (lane >> 1) & 1, entry = 2 * (lane >> 2) + W;
    if (lane < 2 * K) s = block_sum_segment_component(lds + entry * kTeamRowDoubles + 34 * seg + comp);
    s += dpp_mov_f64<kDppQuadXor1>(s, s);  // .x + .y (the .y lane: .y + .x, the same bits)
    s += dpp_mov_f64<kDppQuadXor2>(s, s);  // segment 0 + segment 1
    double* tot = lds + K * kTeamRowDoubles + K * phase;
    phase ^= 1;
    if (lane < 2 * K && (lane % 4) == 0) tot[entry] = s;  // the lane whose adds were x + y, then segment 0 + segment 1
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = tot[k];
}

// block_sum_team2 without the slots: wave W reduce-scatters its K / 2 entries (v[k], k % 2 == W, formed in registers) with the exchange
// tree that pairs the lanes as block_sum_segment pairs lane t's slot t (shared/lc_shared.h: wave_reduce_scatter_lds_order), so every
// total has the LDS forms' bits; one lane per entry stores it into the two-phase rows of totals, which are all the LDS this form needs.
// The barrier, the rows' alternation and the K reads are block_sum_team2's.  lds: sum_team2_reg_lds_doubles(K) doubles.
constexpr int sum_team2_reg_lds_doubles(int K) { return 2 * K; }
template <int K, int W>
__device__ __forceinline__ void block_sum_team2_reg(double (&v)[K], double* lds, int lane, int& phase) {
    static_assert(K % 2 == 0 && K <= 32 && (W == 0 || W == 1), "an even number of entries dealt to two waves");
    double w[K / 2];
#pragma unroll
    for (int i = 0; i < K / 2; ++i) w[i] = v[2 * i + W];
    const double s = wave_reduce_scatter_lds_order<K / 2>(w, lane);
    double* tot = lds + K * phase;
    phase ^= 1;
    const int entry = reduce_scatter_lds_order_entry<K / 2>((lane >> 1) & 15);
    if (lane < 32 && (lane & 1) == 0 && entry >= 0) tot[2 * entry + W] = s;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = tot[k];
}

// The same sum for FOUR wavefronts without sending every thread's K values through LDS (4 x 64 x K doubles each way: the LDS form
// above is bandwidth-bound there, ~2.0 k cycles per sum of 28): each wavefront reduce-scatters its K values in registers
// (permlane / DPP exchanges, the data halves at every step), 16 of its lanes put its 32 wave totals into LDS, 32 threads add the four
// rows in wave order, every thread reads the totals.  Two barriers per sum: the totals alternate between two LDS rows (`phase`,
// toggled by the call), so a wave still reading the previous totals is never overwritten.  lds: at least 4 * 32 + 2 * 32 doubles.
// (Measured with scripts/ubench/wide_stamps.py.)
template <int K>
__device__ __forceinline__ void block_sum_waves4(double (&v)[K], double* lds, int tid, int& phase) {
    static_assert(K <= 32, "one reduce-scatter of 32");
    const int lane = tid & 63, wave = tid >> 6;
    double w[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) w[k] = k < K ? v[k] : 0.0;
    wave_reduce_scatter16<32>(w, lane);
    double* part = lds;                      // [4][32]
    double* tot = lds + 128 + 32 * phase;    // [2][32]
    phase ^= 1;
    if ((lane & 3) == 0) *reinterpret_cast<double2*>(part + 32 * wave + scatter16_base(lane, 2)) = make_double2(w[0], w[1]);
    __syncthreads();
    if (tid < 32) tot[tid] = ((part[tid] + part[32 + tid]) + part[64 + tid]) + part[96 + tid];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = tot[k];
}

// The same sum across the G workgroups that share ONE pose (lc_pnp.hip: lc_pnp_lm_split_kernel -- a batch of few poses with thousands of
// correspondences each leaves three quarters of the chip idle at one workgroup per pose).  Every workgroup reduces its own share as above
// and hands its 32 partial totals to the others through the pose's exchange rows in global memory; each then adds the G rows IN PART ORDER,
// so all of them continue with the same bits and take the same branches of the solve.
// The hand-off is one write and one (polled) read, no counter and no fence: a total travels as two 8-byte words {32 bits of the double,
// 32-bit ticket}, each stored and loaded as ONE agent-scope atomic, and a reader takes a word when it carries the ticket of the sum it is
// waiting for.  Tickets count the sums of a pose over the life of the workspace: `epoch` (a word of the pose's region) holds the ticket of
// the last sum of the previous launch; every part reads it on entry, part 0 writes the new value when it leaves (no part can still be
// waiting to read the old one: part 0 only gets through its first sum after every part has contributed, i.e. has read it).  A slot is
// rewritten every second sum (two rows, by sum parity: a workgroup can be one sum ahead of the slowest, not two -- it cannot finish sum s+1
// before every part has written its s+1 words, i.e. finished reading the rows of sum s), so what a reader finds there is older than the
// ticket it waits for, or it.  Zeroed workspace = ticket 0 everywhere, first sum = ticket 1.
// The wait is bounded in TIME (kSplitWaitTicks of the constant 100 MHz s_memrealtime clock = LC_SPLIT_WAIT_US microseconds, the same budget
// for every split form whatever its polling loop costs; the clock is read once every 16 unsuccessful polls, never on the path of a hand-off
// that arrives) and NOTHING depends on the parts being resident together: a part that has waited
// that long stops for good -- it writes no further exchange word -- and raises the pose's `dirty` word; part 0, whose sums decide the solve
// and which alone stores the pose, reports status 2 ("a part never arrived") when IT ran out of patience.  The rescue launch that follows
// every split launch on the same stream (lc_pnp.hip: lc_pnp_lm_split_rescue_kernel; all parts have ended by then, there are no stragglers)
// re-zeroes the region of a dirty pose -- tickets and epoch start over, so whatever height the abandoned launch left behind cannot be taken
// for a current word -- and re-solves a pose of status 2 with ONE workgroup that plays the G parts one after the other: the same per-thread
// shares, the same wave / workgroup / part order of every sum (block_sum_parts_serial below), hence the bits the parts would have produced.
// So co-residency (pnp_split_parts() sizes grids to at most one workgroup per CU) is what makes the split form FAST; other streams, other
// processes or a CU mask taking compute units away make it slow, never wrong and never different.
// Tail of a pose's region (its last 128 bytes): word 0 epoch, word 1 dirty, word 2 rescues so far (diagnostics: tests read it).
constexpr int kSplitMaxParts = 8;
#ifndef LC_SPLIT_WAIT_US
#define LC_SPLIT_WAIT_US 2000
#endif
constexpr unsigned long long kSplitWaitTicks = 100ull * LC_SPLIT_WAIT_US;
// One unsuccessful poll more: true when the wait's budget is spent.  `t0` = 0 until the first clock read (the 16th unsuccessful poll).
__device__ __forceinline__ bool split_wait_expired(int polls, unsigned long long& t0) {
    if ((polls & 15) != 15) return false;
    const unsigned long long now = __builtin_amdgcn_s_memrealtime();
    if (t0 == 0) { t0 = now; return false; }
    return now - t0 > kSplitWaitTicks;
}
constexpr int kSplitRowWords = 64;                                                             // 32 totals x 2 words
constexpr size_t kSplitPoseBytes = 2 * kSplitMaxParts * kSplitRowWords * sizeof(unsigned long long) + 128;  // two rows per part + the tail's line
constexpr int kSplitLdsDoubles = 128 + 64 + 2;
constexpr int kSplitSerialLdsDoubles = 128 + 32 * kSplitMaxParts + 32;  // block_sum_parts_serial: wave rows, one row per part, the totals
struct SplitSum {
    unsigned long long* exch;  // this pose's [2][kSplitMaxParts][64] words
    unsigned* epoch;           // this pose's tail: epoch, dirty, rescues
    int G, part;
    unsigned base;             // *epoch on entry
    unsigned seq;              // sums finished in this launch
    bool timed_out;
};
__device__ __forceinline__ unsigned* split_tail(void* region, size_t region_bytes) {
    return reinterpret_cast<unsigned*>(static_cast<char*>(region) + region_bytes - 128);
}
__device__ __forceinline__ SplitSum split_sum_enter(void* pose_region, int G, int part) {
    unsigned* epoch = split_tail(pose_region, kSplitPoseBytes);
    return SplitSum{reinterpret_cast<unsigned long long*>(pose_region), epoch, G, part, xcd_load(epoch), 0u, false};
}
// one thread of every part, after its last sum: part 0 of a launch that met every time moves the epoch on; a part that gave up marks the region
__device__ __forceinline__ void split_sum_leave(const SplitSum& sx) {
    if (sx.timed_out) xcd_store(sx.epoch + 1, 1u);
    else if (sx.part == 0 && sx.seq > 0) xcd_store(sx.epoch, sx.base + sx.seq);
}
// The rescue launch's entry, all threads of the workgroup that owns the region: false = nothing to do here.  A dirty region is zeroed
// (every word, the tail's rescue counter excepted); `redo` = the unit has to be computed again by this workgroup.
__device__ __forceinline__ bool split_rescue_enter(void* region, size_t region_bytes, bool redo, int tid, int threads) {
    unsigned* tail = split_tail(region, region_bytes);
    const bool dirty = xcd_load(tail + 1) != 0u;
    if (!dirty && !redo) return false;
    __syncthreads();  // every thread has read the tail before it is rewritten
    if (dirty) {
        unsigned long long* w = static_cast<unsigned long long*>(region);
        for (size_t i = tid; i < (region_bytes - 128) / 8; i += threads) xcd_store(w + i, 0ull);
        if (tid < 2) xcd_store(tail + tid, 0u);
    }
    if (redo && tid == 0) xcd_store(tail + 2, xcd_load(tail + 2) + 1u);
    return redo;
}

template <int K>
__device__ __forceinline__ void block_sum_split(double (&v)[K], double* lds, int tid, int& phase, SplitSum& sx) {
    static_assert(K <= 32, "one reduce-scatter of 32");
    const int lane = tid & 63, wave = tid >> 6;
    double w[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) w[k] = k < K ? v[k] : 0.0;
    wave_reduce_scatter16<32>(w, lane);
    double* part = lds;                      // [4][32]
    double* tot = lds + 128 + 32 * phase;    // [2][32]
    int* arrived_ok = reinterpret_cast<int*>(lds + 192);
    phase ^= 1;
    if (sx.timed_out) {  // (uniform) this part has given up: it stays silent, its caller is on its way out
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] = 0.0;
        return;
    }
    if ((lane & 3) == 0) *reinterpret_cast<double2*>(part + 32 * wave + scatter16_base(lane, 2)) = make_double2(w[0], w[1]);
    __syncthreads();
    if (tid < 32) {
        const unsigned long long ticket = (unsigned long long)(sx.base + sx.seq + 1u) << 32;
        unsigned long long* rows = sx.exch + (size_t)(sx.seq & 1u) * (kSplitMaxParts * kSplitRowWords) + 2 * tid;
        {
            const unsigned long long bits = __builtin_bit_cast(unsigned long long, ((part[tid] + part[32 + tid]) + part[64 + tid]) + part[96 + tid]);
            unsigned long long* mine = rows + sx.part * kSplitRowWords;
            xcd_store(mine, ticket | (bits & 0xFFFFFFFFull));
            xcd_store(mine + 1, ticket | (bits >> 32));
        }
        // all G rows requested at once, again until every word carries the ticket (a row that is already there costs one read)
        unsigned long long lo[kSplitMaxParts], hi[kSplitMaxParts];
        bool ok = true;
        unsigned long long t0 = 0;
        for (int polls = 0;; ++polls) {
#pragma unroll
            for (int g = 0; g < kSplitMaxParts; ++g)
                if (g < sx.G) {
                    lo[g] = xcd_load(rows + g * kSplitRowWords);
                    hi[g] = xcd_load(rows + g * kSplitRowWords + 1);
                }
            unsigned long long late = 0;
#pragma unroll
            for (int g = 0; g < kSplitMaxParts; ++g)
                if (g < sx.G) late |= ((lo[g] ^ ticket) | (hi[g] ^ ticket)) >> 32;
            if (late == 0) break;
            if (split_wait_expired(polls, t0)) { ok = false; break; }
            __builtin_amdgcn_s_sleep(1);
        }
        double s = 0.0;
#pragma unroll
        for (int g = 0; g < kSplitMaxParts; ++g)  // in part order
            if (g < sx.G) s += __builtin_bit_cast(double, (hi[g] << 32) | (lo[g] & 0xFFFFFFFFull));
        tot[tid] = s;
        if (!ok) *arrived_ok = 0;  // (set to 1 by the workgroup before its first sum)
    }
    __syncthreads();
    if (!*arrived_ok) sx.timed_out = true;
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = tot[k];
    ++sx.seq;
}

// block_sum_split played by ONE workgroup for the rescue launch: called once per part g = 0 .. G-1 with the values of that part's share
// (the same threads own the same correspondences as in workgroup g of the split launch), it forms the part's 32 totals exactly as
// block_sum_split does -- wave reduce-scatter, the four wave rows added in wave order -- and keeps them in LDS row g; the call for the last
// part adds the G rows in part order and hands every thread the totals.  lds: kSplitSerialLdsDoubles.
template <int K>
__device__ __forceinline__ void block_sum_parts_serial(double (&v)[K], double* lds, int tid, int g, int G) {
    static_assert(K <= 32, "one reduce-scatter of 32");
    const int lane = tid & 63, wave = tid >> 6;
    double w[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) w[k] = k < K ? v[k] : 0.0;
    wave_reduce_scatter16<32>(w, lane);
    double* part = lds;                               // [4][32]
    double* rows = lds + 128;                         // [G][32]
    double* tot = lds + 128 + 32 * kSplitMaxParts;    // [32]
    if ((lane & 3) == 0) *reinterpret_cast<double2*>(part + 32 * wave + scatter16_base(lane, 2)) = make_double2(w[0], w[1]);
    __syncthreads();
    if (tid < 32) {
        rows[32 * g + tid] = ((part[tid] + part[32 + tid]) + part[64 + tid]) + part[96 + tid];
        if (g == G - 1) {
            double s = 0.0;
            for (int h = 0; h < G; ++h) s += rows[32 * h + tid];  // in part order
            tot[tid] = s;
        }
    }
    __syncthreads();
    if (g == G - 1) {
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] = tot[k];
    }
}

// p z + c as a three-address v_fma_f64 (why: sincos_small below; measured against __builtin_fma with scripts/ubench/pnp_ab.py)
__device__ __forceinline__ double horner_step(double p, double z, double c) {
    double r;
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(r) : "v"(p), "v"(z), "v"(c));
    return r;
}

// sin and cos of a rotation angle 0 <= x <~ 8 (angle-axis norms; the LM keeps them within a few pi): Cody-Waite reduction
// by pi/2 into [-pi/4, pi/4] and the fdlibm minimax polynomials (|error| < 1 ulp on that interval).  About a third of the
// instructions of the general sincos(), whose Payne-Hanek path for huge arguments is never needed here.
// LC_SINCOS_FALLBACK_CALL (set by the latency translation units, whose lone wave per SIMD has registers to spare): the general sincos()
// behind the reduction is a CALL, so that its Payne-Hanek path -- ~190 instructions wherever it is inlined, and sincos_small sits in every
// evaluation of the LM loop -- exists once per code object and away from the loop's code.  The occupancy builds keep it inline: a call
// costs them registers around it (and a stack), and their several waves per SIMD hide an instruction-cache miss.
#ifndef LC_SINCOS_FALLBACK_CALL
#define LC_SINCOS_FALLBACK_CALL 0
#endif
#if LC_SINCOS_FALLBACK_CALL
static __device__ __attribute__((noinline, cold)) double2 sincos_full_range(double x) {
    double s, c;
    sincos(x, &s, &c);
    return make_double2(s, c);
}
#endif
static __device__ __forceinline__ void sincos_small(double x, double& s, double& c) {
#if LC_SINCOS_FALLBACK_CALL
    if (__builtin_expect(!(x < 1.0e4), 0)) {  // wave-uniform and never taken in practice: keep full-range correctness anyway
        const double2 sc = sincos_full_range(x);
        s = sc.x;
        c = sc.y;
        return;
    }
#else
    if (!(x < 1.0e4)) {  // wave-uniform and never taken in practice: keep full-range correctness anyway
        sincos(x, &s, &c);
        return;
    }
#endif
    const double kf = __builtin_rint(x * 0.63661977236758134308);  // x * 2/pi
    const int q = (int)kf;
    double r = __builtin_fma(-kf, 1.57079632673412561417e+00, x);   // pi/2 split in three parts (fdlibm pio2_1, _2, _3)
    r = __builtin_fma(-kf, 6.07710050650619224932e-11, r);
    r = __builtin_fma(-kf, 2.02226624879595063154e-21, r);
    const double z = r * r;
    // sin(r) ~ r + r^3 (S1 + z (S2 + ... )),  cos(r) ~ 1 - z/2 + z^2 (C1 + z (C2 + ...))   (fdlibm k_sin.c / k_cos.c)
    // Horner steps p z + C with the coefficient as the ADDEND: written as three-address v_fma_f64 with C in a register pair that stays
    // live across the LM loop -- the compiler's own form is `v_mov_b64 tmp, C; v_fmac_f64 tmp, z, p` (the accumulating two-address
    // encoding needs the addend in the destination), one extra VALU issue slot per coefficient and evaluation
    double ps = horner_step(1.58969099521155010221e-10, z, -2.50507602534068634195e-08);
    ps = horner_step(ps, z, 2.75573137070700676789e-06);
    ps = horner_step(ps, z, -1.98412698298579493134e-04);
    ps = horner_step(ps, z, 8.33333333332248946124e-03);
    ps = horner_step(ps, z, -1.66666666666666324348e-01);
    const double sr = __builtin_fma(ps * z, r, r);
    double pc = horner_step(-1.13596475577881948265e-11, z, 2.08757232129817482790e-09);
    pc = horner_step(pc, z, -2.75573143513906633035e-07);
    pc = horner_step(pc, z, 2.48015872894767294178e-05);
    pc = horner_step(pc, z, -1.38888888888741095749e-03);
    pc = horner_step(pc, z, 4.16666666666666019037e-02);
    const double cr = __builtin_fma(pc * z, z, __builtin_fma(-0.5, z, 1.0));
    const double ss = (q & 1) ? cr : sr, cc = (q & 1) ? sr : cr;
    s = (q & 2) ? -ss : ss;
    c = ((q + 1) & 2) ? -cc : cc;
}

// atan(s / c) for s >= 0, c >= 0 (not both zero), result in [0, pi/2]: two argument halvings t -> t / (1 + sqrt(1 + t^2))
// (atan t = 2 atan of that) bring the ratio of the smaller to the larger below 0.199, where the odd Taylor series through z^21
// is exact to 2e-17 relative; measured against libm over 2e6 quaternions incl. tiny and half-turn rotations: <= 7e-16 relative (scripts/ubench/atan_accuracy.cpp).
// About a third of the instructions of libm's atan2, which sits on the start-up path of every PnP solve.
__device__ __forceinline__ double atan_ratio_pos(double s, double c) {
    const bool swap = s > c;
    const double a = swap ? c : s, b = swap ? s : c;
    double t = a * fast_rcp(b);  // in [0, 1]
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const double h = fast_sqrt(__builtin_fma(t, t, 1.0));
        t = t * fast_rcp(1.0 + h);
    }
    const double w = t * t;
    double p = horner_step(-1.0 / 21.0, w, 1.0 / 19.0);
    p = horner_step(p, w, -1.0 / 17.0);
    p = horner_step(p, w, 1.0 / 15.0);
    p = horner_step(p, w, -1.0 / 13.0);
    p = horner_step(p, w, 1.0 / 11.0);
    p = horner_step(p, w, -1.0 / 9.0);
    p = horner_step(p, w, 1.0 / 7.0);
    p = horner_step(p, w, -1.0 / 5.0);
    p = horner_step(p, w, 1.0 / 3.0);
    const double at = 4.0 * __builtin_fma(-(p * w), t, t);  // 4 * (t - t^3 (1/3 - t^2/5 + ...))
    return swap ? 1.57079632679489661923 - at : at;
}

// A condition that is the same in every lane, as a SCALAR: lets hipcc branch with s_cbranch instead of saving/masking EXEC
// around code the whole wave takes or skips together (the LM loop's tests on wave-uniform doubles).
__device__ __forceinline__ bool uniform(bool c) { return __builtin_amdgcn_ballot_w64(c) != 0ull; }

}  // namespace lc
