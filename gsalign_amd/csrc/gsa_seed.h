// gsalign_amd/csrc/gsa_seed.h -- device helpers and constants that the seed-search kernels (k_seed.hip, k_seed_dense.hip), the hit
// selection (k_seed_select.hip) and the builders of the index tables (k_tables.hip) share.
#ifndef GSA_SEED_H
#define GSA_SEED_H
#include "gsa_internal.h"

// the device counters of stage 1 (gsa_ctx::d_cnt; the last workgroup of a search kernel copies them to h_cnt)
enum { CNT_OCCBLK = 0, CNT_DONE = 1, CNT_HITS = 2, CNT_SEEDS = 3, CNT_DPCELLS = 4, CNT_DPJOBS = 5, CNT_DPMN = 6, CNT_CAND = 8, CNT_OVERFLOW = 9, CNT_OCCBLK_ALL = 10, CNT_HEAVY = 12 };
#define PATH_WORDS 320          // 10240 on-path bits per chunk
#define QP_WORDS (GSA_CHUNK / 16 + 4)
#define QN_WORDS (GSA_CHUNK / 32 + 4)
// what a lane of a search kernel is waiting for
enum { M_DONE = 0, M_FM = 1, M_TEXT = 2, M_KMER = 3, M_LOC = 4, M_ADV = 5, M_KLO = 6 };

// ---- 2-bit packed sequences: base p sits at bits (2*(p&15)) of word p>>4 (LSB first) ----
__device__ __forceinline__ int q_code(const u32 *qp, int p) { return (qp[p >> 4] >> ((p & 15) << 1)) & 3; }
// (on = false: the chunk has no ambiguous base and keeps no N bitmap -- see SeedLds; the answer is 0 without a read)
__device__ __forceinline__ int q_isn(const u32 *qn, int p, bool on = true) { return on ? (qn[p >> 5] >> (p & 31)) & 1 : 0; }
__device__ __forceinline__ u64 funnel64(u32 w0, u32 w1, u32 w2, int sh)      // 64 bits starting sh (even, < 32) bits into w0
{
	const u64 lo = (u64)w0 | ((u64)w1 << 32);
	return sh ? (lo >> sh) | ((u64)w2 << (64 - sh)) : lo;
}
__device__ __forceinline__ u64 q_bits64(const u32 *qp, int p) { const int w = p >> 4; return funnel64(qp[w], qp[w + 1], qp[w + 2], (p & 15) << 1); }
__device__ __forceinline__ u32 q_nbits32(const u32 *qn, int p, bool on = true) { if (!on) return 0u; const int w = p >> 5; return (u32)((((u64)qn[w + 1] << 32) | qn[w]) >> (p & 31)); }

// Unique interval (x2 == 1): how many of the next (at most 32) query bases continue the only
// occurrence, i.e. pos+t < clen, tp+t < tend, query base t unambiguous and equal to text base t.
// Equivalent to that many successful bwt_2occ4 steps, which leave x0 and x2 = 1 unchanged
// (see DESIGN.md section 4).  r0..r2 = packed reference words starting at word tp>>4.
__device__ __forceinline__ int text_match32(u32 r0, u32 r1, u32 r2, i64 tp, i64 tend, const u32 *qp, const u32 *qn, int pos, int clen, bool qn_on = true)
{
	int avail = clen - pos;
	if (tend - tp < (i64)avail) avail = (int)(tend - tp);
	if (avail > 32) avail = 32;
	if (avail <= 0) return 0;
	const u64 d = funnel64(r0, r1, r2, (int)(tp & 15) << 1) ^ q_bits64(qp, pos);
	const u64 dm = (d | (d >> 1)) & 0x5555555555555555ull;
	const u32 nm = q_nbits32(qn, pos, qn_on);
	int n = dm ? (__ffsll((unsigned long long)dm) - 1) >> 1 : 32;
	const int fn = nm ? __ffs((int)nm) - 1 : 32;
	n = n < fn ? n : fn;
	return n < avail ? n : avail;
}

// Presence table: does a pres_k-mer occur in the indexed text?  BWT_Search from s reaches MinSeedLength iff the first
// MinSeedLength bases occur, so an absent pres_k-mer (pres_k <= MinSeedLength) settles a search that yields no seed with ONE read.
// GROUPED layout (round 3): a walk crosses the ~14 starts in front of a mismatch one by one, so the kernel asks about s, s+1,
// s+2, s+3 together -- as a plain bitmap indexed by the k-mer those were four reads of four unrelated cache lines (most of the
// seed kernel's 6.2 GB of fetches per 250 Mb contig, profiles/archive/r02_pmc_human.json).  The four k-mers share the K-3 bases
// q[s+3 .. s+K): that CORE selects a 32-byte line, and bit 64 i + e_i of the line answers for start s+i, where e_i (6 bits) are
// the three bases of that k-mer outside the core -- q[s+i .. s+3) and q[s+K .. s+K+i).  A k-mer of the text is therefore entered
// four times, once per role i.  4^(K-3) lines: 512 MiB for K = 15.  (pres4_line / pres4_bits take the query's 2-bit window from
// the group's first base; the builder derives the same numbers from the k-mer alone.)
__device__ __forceinline__ u32 pres4_line(u64 qb, int K) { return (u32)((qb >> 6) & ((1ull << (2 * (K - 3))) - 1)); }
__device__ __forceinline__ u32 pres4_bit(u64 qb, int K, int i)      // 0 .. 255: position inside the line for start s + i
{
	const u32 head = (u32)(qb >> (2 * i)) & ((1u << (2 * (3 - i))) - 1);          // q[s+i .. s+3)
	const u32 tail = (u32)(qb >> (2 * K)) & ((1u << (2 * i)) - 1);                // q[s+K .. s+K+i)
	return (u32)i * 64u + (head | (tail << (2 * (3 - i))));
}

// Exclusive prefix of the per-chunk hit counts (n1 = chunks + 1 entries, the last one is 0), by the workgroup that is through
// LAST in a seed kernel: the counts were stored with agent-scope atomics and are read the same way (the other workgroups ran on
// other XCDs), 8 or 16 loads in flight per lane.  Was a rocPRIM scan behind the kernel: two more GPU operations per contig.
template <int TPB>
__device__ __forceinline__ void wg_exscan_hits(const i32 *hits, i32 *base, int n1)
{
	constexpr int V = TPB <= 64 ? 16 : 8;             // loads in flight per lane
	__shared__ i32 s_ws[TPB / 64], s_run;
	const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
	if (tid == 0) s_run = 0;
	__syncthreads();
	for (int b0 = 0; b0 < n1; b0 += TPB * V) {
		i32 v[V], tsum = 0;
#pragma unroll
		for (int k = 0; k < V; k++) { const int idx = b0 + tid * V + k; v[k] = idx < n1 ? __hip_atomic_load(&hits[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0; }
#pragma unroll
		for (int k = 0; k < V; k++) tsum += v[k];
		i32 inc = tsum;
		for (int o = 1; o < 64; o <<= 1) { const i32 t = __shfl_up(inc, o); if (lane >= o) inc += t; }
		if (lane == 63) s_ws[wv] = inc;
		__syncthreads();
		i32 wo = 0, tot = 0;
		for (int w = 0; w < TPB / 64; w++) { const i32 x = s_ws[w]; if (w < wv) wo += x; tot += x; }
		i32 e = s_run + wo + inc - tsum;
#pragma unroll
		for (int k = 0; k < V; k++) { const int idx = b0 + tid * V + k; if (idx < n1) base[idx] = e; e += v[k]; }
		__syncthreads();
		if (tid == 0) s_run += tot;
		__syncthreads();
	}
}

// The same by ONE WAVE of a workgroup whose other waves are busy with chunks of their own (k_seed_wg with SEED_WPW > 1): no LDS, no workgroup barrier.
__device__ __forceinline__ void wave_exscan_hits(const i32 *hits, i32 *base, int n1)
{
	constexpr int V = 16;
	const int lane = threadIdx.x & 63;
	i32 run = 0;
	for (int b0 = 0; b0 < n1; b0 += 64 * V) {
		i32 v[V], tsum = 0;
#pragma unroll
		for (int k = 0; k < V; k++) { const int idx = b0 + lane * V + k; v[k] = idx < n1 ? __hip_atomic_load(&hits[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0; }
#pragma unroll
		for (int k = 0; k < V; k++) tsum += v[k];
		i32 inc = tsum;
		for (int o = 1; o < 64; o <<= 1) { const i32 t = __shfl_up(inc, o); if (lane >= o) inc += t; }
		i32 e = run + inc - tsum;
#pragma unroll
		for (int k = 0; k < V; k++) { const int idx = b0 + lane * V + k; if (idx < n1) base[idx] = e; e += v[k]; }
		run += __shfl(inc, 63);
	}
}

// Four ASCII bases (one dword, first base in the low byte) -> their nt4 codes packed LSB first in bits 0-7 (an ambiguous base: code 0,
// as gsa_nt4's 4 & 3) | the "ambiguous" flags of the four in bits 8-11.  gsa_nt4 (nst_nt4_table, bntseq.c:40-57) byte by byte costs
// ~17 VALU instructions per base; staging a 10 000-base chunk that way was a tenth of the seed kernel's instructions.  Here: fold the
// case, code = ((b >> 1) & 3) ^ (its own high bit) -- a 0, c 1, g 3 ^ 1 = 2, t 2 ^ 1 = 3 -- look the letter that code stands for up with
// one v_perm and compare: anything that is not that letter is ambiguous.  ~5 instructions per base.
__device__ __forceinline__ u32 nt4_quad(u32 w)
{
	const u32 l = w | 0x20202020u;
	const u32 x = (l >> 1) & 0x03030303u;
	u32 code = x ^ ((x >> 1) & 0x01010101u);
	const u32 want = __builtin_amdgcn_perm(0u, 0x74676361u, code);               // bytes 'a' 'c' 'g' 't' selected by the four codes
	const u32 diff = l ^ want;
	const u32 bad = ((diff | ((diff & 0x7f7f7f7fu) + 0x7f7f7f7fu)) >> 7) & 0x01010101u;      // 1 per byte that is not the letter of its code
	code &= ~(bad * 3u);
	return ((code * 0x01041040u) >> 24) | (((bad * 0x01020408u) >> 24) & 15u) << 8;
}

// 32 bases from `src` (position p0 of a chunk of clen bases; behind the chunk: N) -> two words of 2-bit codes + the word of their N flags
__device__ __forceinline__ void stage32(const uint8_t *src, int p0, int clen, u32 &w0, u32 &w1, u32 &wn)
{
	u32 d[8];
	if (p0 + 32 <= clen) { const uint4 a = *(const uint4 *)src, b = *(const uint4 *)(src + 16); d[0] = a.x; d[1] = a.y; d[2] = a.z; d[3] = a.w; d[4] = b.x; d[5] = b.y; d[6] = b.z; d[7] = b.w; }
	else {
#pragma unroll
		for (int t = 0; t < 8; t++) { d[t] = 0; for (int k = 0; k < 4; k++) d[t] |= (u32)(p0 + 4 * t + k < clen ? src[4 * t + k] : (uint8_t)'N') << (8 * k); }
	}
	w0 = w1 = wn = 0;
#pragma unroll
	for (int t = 0; t < 8; t++) {
		const u32 r = nt4_quad(d[t]);
		if (t < 4) w0 |= (r & 0xffu) << (8 * t); else w1 |= (r & 0xffu) << (8 * (t - 4));
		wn |= (r >> 8) << (4 * t);
	}
}

#endif
