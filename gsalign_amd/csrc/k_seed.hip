// gsalign_amd/csrc/k_seed.hip -- stage 1: seed exploration (a4, a5) by the speculative kernel, and the stage's host driver.
// The dense fallback is k_seed_dense.hip; locate (a3), the ordering by (PosDiff, qPos) and SeedGrouping (a6) are k_seed_select.hip.
//
// Replaces IdentifyLocalMEM + BWT_Search
// (reference src/GSAlign.cpp:51-107; src/bwt_search.cpp:121-185).
#include <cstring>
#include <mutex>
#include <condition_variable>
#include <vector>
#include "gsa_ctx.h"
#include "gsa_fm.h"
#include "gsa_scan.h"
#include "gsa_seed.h"

#define SEED_WG 64              // lanes per chunk: ONE WAVE, and the kernel says so (threadIdx.x & 63, >> 6).  (128 lanes = two waves per chunk spent 27 % more VALU
                                // wave-instructions on the same searches -- a wave iterates as long as its slowest lane: profiles/archive/r03_seed_shape_sweep.txt)
#ifndef NSUB
#define NSUB 64                // sub-ranges per chunk (work items of the wave, drawn from an LDS queue): ONE per lane.  A sub-range is only where a walk STARTS -- walks
                               // cross sub-range ends until they meet memoised or claimed ground -- so every further one is one more speculative search (96 -> 64: a sixth
                               // fewer requests per chunk), and the kernel is bound by its requests.  Swept 48 .. 96 on the bench: 64 wins by 4 % (profiles/seed_claims_ab.txt;
                               // while walks stopped at sub-range ends 96 was best, and 64 is within 1 % of it there)
#endif
#ifndef ADV_STEPS
#define ADV_STEPS 4             // advance steps (taking an item, steps over ambiguous positions, opening a search) per round trip
#endif
#ifndef PLOOK
#define PLOOK 3                 // presence bits looked up beside the one of the current start
#endif

// ---------------------------------------------------------------------------
// Seed exploration.  Work unit = one 10 000-bp chunk (absolute position, App. B
// #1).  Inside a chunk the reference walks a CHAIN: next start = start+len+1
// after an accepted match (start+5 with -sen), start+1 otherwise, so the walk is
// sequential -- but "next start" is a pure function of the start position, i.e.
// the chunk is a functional graph whose paths merge (two walks that are inside
// the same exact match end at the same mismatch).  One WAVE owns a chunk and
// cuts it into NSUB sub-ranges.  The pass: lanes pull sub-ranges from an
// LDS queue and walk from each one's left edge, memoising next(s) per position.
// A walk goes on ACROSS sub-range ends until the start it arrives at is memoised,
// CLAIMED by a search in flight (a bit per start, set when the search is opened)
// or behind the chunk's end; then the lane takes the next sub-range.  Item 0
// claims start 0, and whoever completes the search at a chain position claims the
// next one or finds it claimed or memoised: when the pass is over the whole true
// chain is memoised, and so is the memo path from every left edge.  The resolver
// behind the pass reads LDS only: the exit of every sub-range along the memo,
// the sub-ranges on the chain by pointer jumping, the exits of those from their
// true entries, until no exit moves.  (A start it meets unsearched -- the claims
// say that there is none -- gets a fallback pass of the loop.)  The result is
// exactly the reference's chain; the on-path bit per position selects which
// memoised matches become seeds.  Query (2-bit packed + N bitmap), memo, claims and
// exits live in LDS; so do the on-path bits, in the query's words once the walks are over.
// ---------------------------------------------------------------------------

#ifndef SEED_MIN_WAVES
#define SEED_MIN_WAVES 5        // waves per SIMD the register allocation must allow: 5 = 96 VGPRs (the loop wants ~150: some 40 live in ~200 bytes of scratch).  Round 6: what the
                                // kernel leaves FREE on a CU is worth more than what the spills cost it -- see k_seed_wg.  (3 until round 6: 149 VGPRs, no scratch.)
#endif
// SEED_LDS_DIET = 1 (an experiment build, NOT the product: DESIGN.md section 8e): a chunk's LDS state cut from 12.0 KB to 9.0 KB -- 512 long-hop entries, and
// only a chunk with an ambiguous base keeps an N bitmap, in the place of half of them -- so that eleven waves fit the LDS that eight take.
#ifndef SEED_LDS_DIET
#define SEED_LDS_DIET 0
#endif
#ifndef LHOP_N
#define LHOP_N (SEED_LDS_DIET ? 512 : 1024)      // entries of the long-hop table
#endif
#ifndef LHOP_NN
#define LHOP_NN (SEED_LDS_DIET ? 256 : LHOP_N)   // ... of a chunk WITH ambiguous bases under the diet; the N bitmap lies behind them (the product: behind the whole table)
#endif
#define LHOP_WORDS (LHOP_NN + QN_WORDS > LHOP_N ? LHOP_NN + QN_WORDS : LHOP_N)
static_assert((LHOP_N & (LHOP_N - 1)) == 0 && (LHOP_NN & (LHOP_NN - 1)) == 0 && LHOP_NN <= LHOP_N, "the long-hop table is indexed with a mask");
// next(s) - s per position of a chunk, two bits each.  Lanes set different codes of one word at the same time (atomic OR); a position is only ever given ONE
// value (next(s) is a function of s), so setting it twice is harmless.  next(s) - s only ever takes three kinds of value -- 1 (no seed from s), 5 (an accepted match under -sen:
// GSAlign.cpp:88-91) and len + 1 >= MinSeedLength + 1 (an accepted match) -- so the codes are 0 unknown, 1 -> +1, 2 -> +5, 3 -> the hop sits in the
// hash table; anything else (hops of 2-4, 6-...: the accounting build, MinSeedLength below 5) goes to the table as well.  5 KB -> 2.5 KB per chunk:
// LDS x time is what the seed kernel costs the chip (a CU's LDS holds its chunks and nothing else's meanwhile), see DESIGN section 4.
#define MEMO_WORDS (GSA_CHUNK / 16)
__device__ __forceinline__ int memo_nib(const u32 *memo, int s) { return (int)((memo[s >> 4] >> ((s & 15) << 1)) & 3u); }      // the code: 0 = unknown
__device__ __forceinline__ void memo_one(u32 *memo, int s) { atomicOr(&memo[s >> 4], 1u << ((s & 15) << 1)); }
__device__ __forceinline__ int memo_get(const u32 *memo, const u32 *lhop, u32 lmask, int s)
{
	const int v = memo_nib(memo, s);
	if (v < 2) return v;
	if (v == 2) return 5;
	for (u32 h = ((u32)s * 40503u) >> 6;; h++) { const u32 e = lhop[h & lmask]; if ((e >> 16) == (u32)s + 1) return (int)(e & 0xffffu); }
}
__device__ __forceinline__ void memo_set(u32 *memo, u32 *lhop, u32 lmask, int s, int d, int *abort_flag)
{
	if (d == 1 || d == 5) { atomicOr(&memo[s >> 4], (d == 1 ? 1u : 2u) << ((s & 15) << 1)); return; }
	const u32 e = ((u32)(s + 1) << 16) | (u32)d;
	u32 h = ((u32)s * 40503u) >> 6;
	for (u32 tries = 0; tries <= lmask; tries++, h++) {
		const u32 old = atomicCAS(&lhop[h & lmask], 0u, e);
		if (old == 0 || old == e) { atomicOr(&memo[s >> 4], 3u << ((s & 15) << 1)); return; }      // (two walks that reach the same start store the same hop: next(s) is a function of s)
	}
	*(volatile int *)abort_flag = 1;                                // table full: the chunk is redone by the dense kernels
}
// The memo path from s to the first position at or behind `end` (LDS reads only); -1 where it meets a start nobody has searched, which `unk` then names.
__device__ __forceinline__ int memo_trace(const u32 *memo, const u32 *lhop, u32 lmask, int s, int end, int &unk)
{
	while (s < end) { const int m = memo_get(memo, lhop, lmask, s); if (!m) { unk = s; return -1; } s += m; }
	return s;
}
#define CLAIM_WORDS ((GSA_CHUNK + 31) / 32)

// Everything a wave keeps in LDS for its chunk.  One object per WAVE: a workgroup of k_seed_wg is SEED_WPW independent waves, each with its own chunk, queue,
// memo and resolver state; nothing in seed_chunk synchronises across waves.  (One chunk per wave, one search per lane: the other shapes that were
// measured are in DESIGN.md section 8f.)
template <bool COUNT>
struct SeedLds {
	u32 s_ncand, s_queue, s_hits;
	int changed, s_abort;
	// The query as 2-bit codes.  Dead once the walks are over: the on-path bitmap (PATH_WORDS words, set by the resolved chain behind the loop) then takes its place.
	u32 qp[QP_WORDS];
	// next(s) - s per position as 2-bit codes + a hash table for the long hops (memo_get / memo_set above); a full table sends the
	// chunk to the dense kernels like an exhausted budget does.
	u32 memo[MEMO_WORDS];
	// (s + 1) << 16 | hop, 0 = free: LHOP_N entries, and behind entry LHOP_NN the N bitmap (QN_WORDS words).  The product: LHOP_NN = LHOP_N, the two simply lie
	// one behind the other.  SEED_LDS_DIET: a chunk without an ambiguous base (nearly all of them) uses all LHOP_N entries and has NO N bitmap -- its flags are all zero
	// and q_nbits32 says so without a read; a chunk with one hashes into the first LHOP_NN entries only.  At 1-2 % divergence a chunk stores 200-300 long hops (its
	// accepted matches plus one per speculative sub-range), so such a chunk's table runs full and may hand the chunk over: the slower, still exact road.
	u32 lhop[LHOP_WORDS];
	uint16_t mblk[COUNT ? GSA_CHUNK : 1];   // Occ blocks the search from s read (accounting build only)
	uint16_t entry_of[NSUB], exit_of[NSUB];             // the resolver's: true entry of an on-chain sub-range; where the memo path from its entry leaves it
	uint16_t pend_s[SEED_WG];                           // starts the resolver met unsearched: a fallback pass of the loop begins there
	uint16_t jmp[2][NSUB];                              // pointer-jumping buffers
	// One bit per start: a search from it has been opened in this pass (atomicOr; the old value decides who searches).  A walk that arrives at a claimed start leaves
	// it to its owner and takes other work, so no start is searched twice and no accepted match is entered twice.
	u32 claim[CLAIM_WORDS];
	u32 onchain[(NSUB + 31) / 32], s_npend;
	int s_last;
};
// A wave's own synchronisation point.  One wave per workgroup: __syncthreads() as ever (the barrier itself is elided for a one-wave workgroup, the fences
// stay).  Several: the waves are independent, and LDS operations of ONE wave are performed in the order they were issued, so all that is needed is that
// the compiler keeps that order.
#define SEED_SYNC() do { if (WPW == 1) __syncthreads(); else { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } } while (0)
template <bool COUNT, bool E16, int WPW>
__device__ __forceinline__ void seed_chunk(const DevIndex &di, const uint8_t *__restrict__ q, i32 qlen, const Params &prm, u64 *cnt,
                                                      i32 *cand_s, i32 *cand_len, u64 *cand_x0, i32 *cand_freq, u32 cand_cap, u32 *cand_cnt, u32 *onpath, i32 *chunk_hits, u64 *hcnt,
                                                      u32 budget, u32 *heavy_list, i32 *chunk_base, const int chunk, const u32 n_chunks, const u32 lhop_cap, SeedLds<COUNT> &L)
{
	const int j = threadIdx.x & 63;      // (lane: a workgroup is SEED_WPW independent waves)
	const i64 c0 = (i64)chunk * GSA_CHUNK;
	const int clen = (int)((i64)qlen - c0 < GSA_CHUNK ? (i64)qlen - c0 : GSA_CHUNK);
	const int S0 = (clen + NSUB - 1) / NSUB, S = S0 < 1 ? 1 : S0;       // sub-range length
	const int nitems = (clen + S - 1) / S;
	const size_t cbase = (size_t)chunk * cand_cap;           // this chunk's private candidate segment
	// stage the chunk: 32 bases per lane per pass -> two code words + one N word (16-byte global loads)
	// (the N words go into the zeroed hop table's tail, and only those that have a flag set: hence the table first)
	for (int p = j; p < MEMO_WORDS; p += SEED_WG) L.memo[p] = 0;
	for (int p = j; p < LHOP_WORDS; p += SEED_WG) L.lhop[p] = 0;
	for (int p = j; p < CLAIM_WORDS; p += SEED_WG) L.claim[p] = 0;
	if (j == 0) { L.s_ncand = 0; L.s_hits = 0; }
	SEED_SYNC();
	bool anyn = false;
	for (int g = j; g < QN_WORDS; g += SEED_WG) {
		u32 w0 = 0, w1 = 0, wn = 0;
		const int p0 = g << 5;
		if (p0 < clen) stage32(q + c0 + p0, p0, clen, w0, w1, wn);
		if (2 * g < QP_WORDS) L.qp[2 * g] = w0;
		if (2 * g + 1 < QP_WORDS) L.qp[2 * g + 1] = w1;
		// (stage32 flags the positions behind the chunk's end as N.  Nobody asks about those -- every reader bounds itself by clen first -- and
		//  they must not make the short last chunk of every contig an N chunk)
		if (p0 + 32 > clen) wn = p0 < clen ? wn & ((1u << (clen - p0)) - 1u) : 0u;
		if (wn) { L.lhop[LHOP_NN + g] = wn; anyn = true; }
	}
	const bool hasn = !SEED_LDS_DIET || __any(anyn);      // (wave-uniform) the chunk has an ambiguous base: N bitmap behind LHOP_NN hop entries (the product reads the bitmap whatever it holds)
	const u32 *const qn = &L.lhop[LHOP_NN];
	// (lhop_cap: a power of two, the entries a test lets the table use -- gsa_set_option "seed_lhop"; LHOP_N otherwise)
	const u32 lmask = (SEED_LDS_DIET && hasn && lhop_cap > (u32)LHOP_NN ? (u32)LHOP_NN : lhop_cap) - 1u;
	if (j == 0) { L.s_queue = 0; L.s_npend = 0; L.s_abort = 0; }
	u32 all_blocks = 0, rounds = 0, iters = 0;
#ifdef SEED_STATS
	u32 st_it = 0, st_pend = 0, st_late = 0, st_act = 0, st_fm = 0;
#endif
	unsigned long long t_begin = wall_clock64(), t_round0 = 0, t_resolve = 0;
	u32 dirty = 0;                                      // a fallback pass: this lane has one start (fb_start) to walk from
	int fb_start = 0;
	SEED_SYNC();
	for (;;) {
		// One flat loop per wave.  Every iteration each lane has exactly ONE memory request pending
		// (two Occ blocks / 12 bytes of packed reference text / a k-mer table entry / an SA entry); all
		// lanes issue their requests together, wait once, then consume by mode -- so lanes that are in
		// different searches, or in different phases of a search, never serialise on each other's
		// memory latency.
		int s = 0, pos = 0, mode = M_ADV; u32 kid = 0, pid = 0, pext = 0;
		int lclen = 0;                                        // the chunk's length once the lane holds an item
		FmIntv ik = {0, 0, 0}; u32 blk = 0; i64 tp = 0;
		bool need_item = true;
		while (!__all(mode == M_DONE)) {
			iters++;
			// A chunk whose walks exceed the budget (a tandem array with more than MaxSeedFreq copies: every start is searched for
			// ~100 bases, rejected and followed by start+1 -- thousands of dependent searches on a handful of lanes) is given up
			// here and searched from EVERY position in parallel by the dense kernels (k_seed_dense.hip).
			if (!COUNT && budget && iters > budget) *(volatile int *)&L.s_abort = 1;
			if (*(volatile int *)&L.s_abort) break;
#ifdef SEED_STATS      // (experiments: what the wave-iterations are spent on -- sums over all waves instead of the maxima / timers)
			{ const u64 bf = __ballot(mode == M_FM), ba = __ballot(mode != M_DONE);
			  st_it++; st_late += rounds != 0; st_act += __popcll(ba); st_fm += __popcll(bf); }
#endif
			// ---- request phase (convergent): every kind of request is issued by every lane; a lane that does not want it reads entry 0 ----
			u64 kk = 0, ll = 0; bool kn = true, ln = true;
			if (mode == M_FM) {
				const u64 k = ik.x1 - 1, l = ik.x1 - 1 + ik.x2;
				kn = (k == (u64)-1); ln = (l == (u64)-1);
				kk = kn ? 0 : k - (k >= di.primary); ll = ln ? 0 : l - (l >= di.primary);
			}
			const FmBlock bk = fm_load(di, kk >> 6), bl = fm_load(di, ll >> 6);
			struct __attribute__((packed, aligned(4))) W5 { u32 a, b, c, d, e; };
			const W5 w5 = *(const W5 *)(di.ref2 + (mode == M_TEXT ? (tp >> 4) : 0));      // 20 bytes of packed text: a 64-base window
			const u32 r0 = w5.a, r1 = w5.b, r2 = w5.c, r3 = w5.d, r4 = w5.e;
			// one k-mer table entry: 16 bytes (one load) when the text is below 2^32, else 32
			ulonglong2 e0 = {0, 0}, e1 = {0, 0};
			if (E16) {
				const uint4 e = ((const uint4 *)(di.kmer ? di.kmer : (const u64 *)di.bwt))[mode == M_KMER ? kid : 0];
				e0.x = e.x; e0.y = e.y; e1.x = e.z; e1.y = e.w;
			} else {
				const ulonglong2 *pe = (const ulonglong2 *)((di.kmer ? di.kmer : (const u64 *)di.bwt) + (mode == M_KMER ? ((size_t)kid << 2) : 0));
				e0 = pe[0]; e1 = pe[1];
			}
			// presence bits of s and of the three starts behind it: a search that dies below MinSeedLength moves on by ONE base,
			// so walks cross the 14 bases in front of a mismatch start by start -- four of those per memory round trip, all four
			// from ONE 32-byte line (pres4_*)
			uint4 pl0 = {~0u, ~0u, ~0u, ~0u}, pl1 = {~0u, ~0u, ~0u, ~0u};
			if (di.pres) { const uint4 *pp = (const uint4 *)di.pres + 2 * (size_t)(mode == M_KMER ? pid : 0); pl0 = pp[0]; pl1 = pp[1]; }
			// (bit 64 i + e_i of the line: dword 2 i + (e_i >> 5).  e_i = pres4_bit(.., i) & 63 = the three bases outside the core = bits 2 i .. 2 i + 5 of
			//  the 12-bit number pext = q[s .. s+3) | q[s+K .. s+K+3) << 6: one number per open search instead of four packed ones)
#define PRES4_TEST(I) ((((((pext >> (2 * (I))) & 32u) ? ((I) == 0 ? pl0.y : (I) == 1 ? pl0.w : (I) == 2 ? pl1.y : pl1.w) : ((I) == 0 ? pl0.x : (I) == 1 ? pl0.z : (I) == 2 ? pl1.x : pl1.z)) >> ((pext >> (2 * (I))) & 31u)) & 1u) != 0)
			const u64 sav = fm_locate(di, mode == M_LOC ? ik.x0 : 1);
			// ---- consume phase: straight-line, one predicated block per mode ----
			bool ended = false;
			if (mode == M_KMER) {
				if (!PRES4_TEST(0)) {                  // the first MinSeedLength bases do not occur: no seed here, next start s+1
					memo_one(L.memo, s); s += 1; mode = M_ADV;
					// ... and the same for the starts behind it, as long as nothing else is known about them (the advance step
					// below owns every other rule: chunk end, memoised or claimed start, ambiguous bases, too close to the chunk end)
					const int ML = prm.MinSeedLength < 32 ? prm.MinSeedLength : 32;
#pragma unroll
					for (int k2 = 0; k2 < PLOOK; k2++) {
						if (s >= lclen || memo_nib(L.memo, s)) break;
						const u32 nb = q_nbits32(qn, s, hasn);
						if (s + prm.MinSeedLength > lclen || (nb & (ML == 32 ? ~0u : (1u << ML) - 1)) != 0) break;
						if (k2 == 0 ? PRES4_TEST(1) : k2 == 1 ? PRES4_TEST(2) : PRES4_TEST(3)) break;          // occurs: needs its table entry (next iteration)
						memo_one(L.memo, s); s += 1;
					}
				} else {
					const bool hit = e1.x != 0;         // absent k-mer: the match is shorter than k, walk it base by base
					if (hit) { ik.x0 = e0.x; ik.x1 = e0.y; ik.x2 = e1.x; pos = s + di.kmer_k; }
					else ik = fm_init(di, q_code(L.qp, s));      // (pos = s + 1 since the search was opened)
					mode = M_FM;
					if (hit && ik.x2 == 1) { tp = (i64)(e1.y - 1) + di.kmer_k; mode = M_TEXT; }      // unique: straight to the text comparison
				}
			} else if (mode == M_LOC) {
				tp = (i64)sav + (pos - s); mode = M_TEXT;
			} else if (mode == M_TEXT) {
				int got = text_match32(r0, r1, r2, tp, (i64)di.seq_len, L.qp, qn, pos, lclen, hasn);
				if (got == 32) got += text_match32(r2, r3, r4, tp + 32, (i64)di.seq_len, L.qp, qn, pos + 32, lclen, hasn);
				pos += got; tp += got;
				ended = got < 64;
			} else if (mode == M_FM) {
				const bool can = pos < lclen && !q_isn(qn, pos < lclen ? pos : 0, hasn);
				const bool ok = can && fm_extend_loaded(di, ik, q_code(L.qp, pos < lclen ? pos : 0), bk, bl, kk, ll, kn, ln, blk);
				ended = !ok;
				if (ok) { pos++; if (!COUNT && ik.x2 == 1) mode = M_LOC; }
			}
			if (ended) {
				const int len = pos - s;
				int d = 1;
				if (len >= prm.MinSeedLength && ik.x2 <= GSA_MAX_SEED_FREQ) {
					const u32 slot = atomicAdd(&L.s_ncand, 1u);                 // LDS counter: no global round trip in the loop
					if (slot < cand_cap) { cand_s[cbase + slot] = (i32)(c0 + s); cand_len[cbase + slot] = len; cand_x0[cbase + slot] = ik.x0; cand_freq[cbase + slot] = (i32)ik.x2; }
					else cnt[CNT_OVERFLOW] = 1;
					d = prm.bSensitive ? 5 : len + 1;
				}
				memo_set(L.memo, L.lhop, lmask, s, d, &L.s_abort); if (COUNT) L.mblk[s] = (uint16_t)blk;
				all_blocks += blk;
				s += d; mode = M_ADV;
			}
			// ---- advance: take an item / step over an ambiguous position / open the next search.  The walk of an item ends where its start is memoised
			// (from there on the memo is the path: the resolver follows it without a memory request), claimed by a search in flight, or behind the chunk's
			// end -- never because a sub-range ends.  No lane waits for a claim: it takes other work.  (A few steps per iteration: none of them costs a memory access) ----
			for (int step = 0; step < ADV_STEPS && mode == M_ADV; step++) {
				if (need_item) {
					if (rounds == 0) { const u32 it_ = atomicAdd(&L.s_queue, 1u); s = it_ < (u32)nitems ? (int)it_ * S : -1; }
					else if (dirty) { dirty = 0; s = fb_start; }
					else s = -1;
					need_item = false;
					if (s < 0) { mode = M_DONE; break; }
					lclen = clen;
				}
				if (s >= lclen || memo_nib(L.memo, s)) { need_item = true; continue; }
				const u32 nb = q_nbits32(qn, s, hasn);
				const int ML = prm.MinSeedLength < 32 ? prm.MinSeedLength : 32;
				if (nb & 1u) { memo_one(L.memo, s); if (COUNT) L.mblk[s] = 0; s += 1; }
				else if (!COUNT && (s + prm.MinSeedLength > lclen || (nb & (ML == 32 ? ~0u : (1u << ML) - 1)) != 0)) { memo_one(L.memo, s); s += 1; }      // cannot reach MinSeedLength
				else {
					const u32 cbit = 1u << (s & 31);
					if (atomicOr(&L.claim[s >> 5], cbit) & cbit) { need_item = true; continue; }      // someone else's search
					pos = s + 1; blk = 0; mode = M_FM;
					// (the interval of the first base -- fm_init: three 5-way selects of 64-bit numbers -- only where the walk really starts
					//  at the first base: next to the chunk end / an N, or behind a k-mer entry that says "absent")
					if (COUNT || !(di.kmer_k > 1 && s + di.kmer_k <= lclen && (nb & ((1u << di.kmer_k) - 1)) == 0)) ik = fm_init(di, q_code(L.qp, s));
					else {
						const u64 qb = q_bits64(L.qp, s);
						kid = (u32)(qb & ((1ull << (2 * di.kmer_k)) - 1)); mode = M_KMER;
						// the line of the presence table that answers for s .. s+3, and the four positions inside it
						pid = di.pres_k ? pres4_line(qb, di.pres_k) : 0;
						pext = di.pres_k ? (((u32)qb & 63u) | (((u32)(qb >> (2 * di.pres_k)) & 63u) << 6)) : 0;
					}
				}
			}
		}
#undef PRES4_TEST
		rounds++;
		SEED_SYNC();
		if (L.s_abort) break;
		if (rounds == 1) t_round0 = wall_clock64() - t_begin;
		const unsigned long long t_r0 = wall_clock64();
		// True entries, from LDS alone.  When the pass is over the memo path from every left edge is complete, so a lane per sub-range follows it to the first
		// position at or behind the sub-range's end: exit_of.  At sub-range level the chain is the orbit of 0 under v -> exit_of[v] / S: found by pointer jumping
		// (log2 NSUB parallel rounds), the true entry of an on-chain sub-range being its predecessor's exit.  A sub-range that is entered elsewhere than its
		// exit was traced from is traced from its true entry; where that moves its exit the chain is resolved again, until no exit moves.  (Sub-range 0 is
		// right from the start, and every round makes the first wrong sub-range of the chain right: at most nitems rounds, one or two in practice.)
		// A trace that meets a start nobody searched -- the claims say there is none -- ends the resolve: those starts are collected, searched in another
		// pass of the loop above (the claims start afresh: every search of the last pass is complete and memoised), and everything is resolved again.
		// Exactness rests on this guard alone, not on the claims.
		if (j == 0) L.s_npend = 0;
		SEED_SYNC();
		for (int v = j; v < NSUB; v += SEED_WG) if (v < nitems) {
			int u = 0;
			const int X = memo_trace(L.memo, L.lhop, lmask, v * S, (v + 1) * S < clen ? (v + 1) * S : clen, u);
			if (X < 0) { const u32 idx = atomicAdd(&L.s_npend, 1u); if (idx < SEED_WG) L.pend_s[idx] = (uint16_t)u; }
			L.exit_of[v] = (uint16_t)(X < 0 ? clen : X);
		}
		SEED_SYNC();
		for (int rr = 0; L.s_npend == 0; rr++) {
			if (rr > nitems) { *(volatile int *)&L.s_abort = 1; break; }      // (cannot happen, see above: the dense kernels are the exact road that is always open)
			for (int v = j; v < NSUB; v += SEED_WG) if (v < nitems) { const int X = L.exit_of[v]; L.jmp[0][v] = (uint16_t)(X >= clen ? 0xffff : X / S); }
			if (j < (NSUB + 31) / 32) L.onchain[j] = 0;
			if (j == 0) L.changed = 0;
			SEED_SYNC();
			if (j == 0) L.onchain[0] = 1u;
			SEED_SYNC();
			int cur = 0;
			for (int span = 1; span < nitems; span <<= 1) {
				for (int v = j; v < NSUB; v += SEED_WG) if (v < nitems) {
					const int t = L.jmp[cur][v];
					if (t != 0xffff) {
						if ((L.onchain[v >> 5] >> (v & 31)) & 1u) atomicOr(&L.onchain[t >> 5], 1u << (t & 31));
						L.jmp[cur ^ 1][v] = L.jmp[cur][t];
					} else L.jmp[cur ^ 1][v] = 0xffff;
				}
				SEED_SYNC();
				cur ^= 1;
			}
			for (int v = j; v < NSUB; v += SEED_WG) if (v < nitems) L.entry_of[v] = (uint16_t)(v ? clen : 0);      // off-chain: nothing to mark
			SEED_SYNC();
			for (int v = j; v < NSUB; v += SEED_WG) if (v < nitems)
				if ((L.onchain[v >> 5] >> (v & 31)) & 1u) { const int X = L.exit_of[v]; if (X < clen) L.entry_of[X / S] = (uint16_t)X; }
			SEED_SYNC();
			for (int v = j; v < NSUB; v += SEED_WG) if (v < nitems) {
				if (!((L.onchain[v >> 5] >> (v & 31)) & 1u)) continue;
				int u = 0;
				const int X = memo_trace(L.memo, L.lhop, lmask, L.entry_of[v], (v + 1) * S < clen ? (v + 1) * S : clen, u);
				if (X < 0) { const u32 idx = atomicAdd(&L.s_npend, 1u); if (idx < SEED_WG) L.pend_s[idx] = (uint16_t)u; }
				else if (X != (int)L.exit_of[v]) { L.exit_of[v] = (uint16_t)X; L.changed = 1; }
			}
			SEED_SYNC();
			const int moved = L.changed;
			SEED_SYNC();
			if (!moved) break;
		}
		const u32 npend = L.s_npend < SEED_WG ? L.s_npend : SEED_WG;
		t_resolve += wall_clock64() - t_r0;
		if (j < (int)npend) { fb_start = L.pend_s[j]; dirty = 1; }
#ifdef SEED_STATS
		st_pend += npend;
#endif
		if (!npend) break;
		for (int p = j; p < CLAIM_WORDS; p += SEED_WG) L.claim[p] = 0;
		SEED_SYNC();
	}
	const bool heavy = L.s_abort != 0;
	if (heavy) {
		if (j == 0) {
			const u32 hslot = (u32)atomicAdd((unsigned long long *)&cnt[CNT_HEAVY], 1ull);
			heavy_list[hslot] = (u32)chunk;
			L.s_ncand = 0; cand_cnt[chunk] = 0; lb_pub(&chunk_hits[chunk], 0); if (chunk == 0) lb_pub(&chunk_hits[n_chunks], 0);
		}
		SEED_SYNC();
	}
	// mark the true path and count the Occ blocks the reference's walk reads.  The walks are over (every way out of the loop is behind a SEED_SYNC), nobody
	// reads the query again: the on-path bits take the first PATH_WORDS words of its place
	static_assert(PATH_WORDS <= QP_WORDS, "the on-path bitmap lies in the query's words");
	u32 *const path = L.qp;
	u32 alg_blocks = 0;
	if (!heavy) {
		for (int p = j; p < PATH_WORDS; p += SEED_WG) path[p] = 0;
		SEED_SYNC();
	}
	if (!heavy) for (int v = j; v < NSUB; v += SEED_WG) if (v < nitems) {
		const int vend = (v + 1) * S < clen ? (v + 1) * S : clen;
		for (int s = L.entry_of[v]; s < vend;) { atomicOr(&path[s >> 5], 1u << (s & 31)); if (COUNT) alg_blocks += L.mblk[s]; s += memo_get(L.memo, L.lhop, lmask, s); }
	}
	for (int o = 32; o; o >>= 1) { alg_blocks += __shfl_down(alg_blocks, o); all_blocks += __shfl_down(all_blocks, o); }
	if (j == 0) {
		if (alg_blocks) atomicAdd((unsigned long long *)&cnt[CNT_OCCBLK], (unsigned long long)alg_blocks);
		if (all_blocks) atomicAdd((unsigned long long *)&cnt[CNT_OCCBLK_ALL], (unsigned long long)all_blocks);
#ifndef SEED_STATS
		atomicMax((unsigned long long *)&cnt[13], (unsigned long long)iters);
#endif
	}
#ifdef SEED_STATS
	if (j == 0) { atomicAdd((unsigned long long *)&cnt[11], (unsigned long long)st_it); atomicAdd((unsigned long long *)&cnt[13], (unsigned long long)st_pend); atomicAdd((unsigned long long *)&cnt[14], (unsigned long long)st_late);
	              atomicAdd((unsigned long long *)&cnt[15], (unsigned long long)st_act); atomicAdd((unsigned long long *)&cnt[7], (unsigned long long)st_fm); }
	if (false)
#endif
	if (j == 0) { atomicMax((unsigned long long *)&cnt[11], (unsigned long long)rounds); atomicMax((unsigned long long *)&cnt[14], t_round0); atomicMax((unsigned long long *)&cnt[15], t_resolve); atomicMax((unsigned long long *)&cnt[7], wall_clock64() - t_begin); }
	SEED_SYNC();
	// the on-path bits, and how many located hits the chunk will contribute (so that the select kernel needs no global atomic)
	if (!heavy) {
		for (int p = j; p < PATH_WORDS; p += SEED_WG) onpath[(size_t)chunk * PATH_WORDS + p] = path[p];
		const u32 nc = L.s_ncand < cand_cap ? L.s_ncand : cand_cap;
		u32 h = 0;
		for (u32 i = j; i < nc; i += SEED_WG) { const i32 p = cand_s[cbase + i] - (i32)c0; if ((path[p >> 5] >> (p & 31)) & 1u) h += (u32)cand_freq[cbase + i]; }
		for (int o = 32; o; o >>= 1) h += __shfl_down(h, o);
		if (j == 0 && h) atomicAdd(&L.s_hits, h);
		SEED_SYNC();
		if (j == 0) {
			cand_cnt[chunk] = nc; lb_pub(&chunk_hits[chunk], (i32)L.s_hits); if (chunk == 0) lb_pub(&chunk_hits[n_chunks], 0); atomicMax((unsigned long long *)&cnt[CNT_CAND], (unsigned long long)L.s_ncand);
			if (L.s_hits) atomicAdd((unsigned long long *)&cnt[CNT_HITS], (unsigned long long)L.s_hits);      // the contig's total: all the host needs to go on
		}
	}
	// the wave that is through last puts the counters into pinned memory (the host waits for this kernel, nothing
	// else) and leaves them at zero for the next contig
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // (every wave: its counter atomics are done before it counts itself)
	SEED_SYNC();
	if (j == 0) {
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");      // (counters are device atomics; an agent-scope fence is an L2 write-back per workgroup here)
		L.s_last = atomicAdd((unsigned long long *)&cnt[CNT_DONE], 1ull) == (unsigned long long)n_chunks - 1ull ? 1 : 0;
	}
	SEED_SYNC();
	if (L.s_last && j < 16) {
		hcnt[j] = j == CNT_DONE ? 0 : __hip_atomic_load(&cnt[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		cnt[j] = 0;
	}
	if (L.s_last) { if (WPW == 1) wg_exscan_hits<SEED_WG>(chunk_hits, chunk_base, (int)n_chunks + 1); else wave_exscan_hits(chunk_hits, chunk_base, (int)n_chunks + 1); }
}
#undef SEED_SYNC


// The kernel: the waves DRAW their chunks from a ticket counter (cnt[SEED_TICKET], never reset: the host passes the value it has at launch, and a launch
// of w waves over n chunks leaves it n + w higher -- every wave's last draw is the one that fails).  The launch is PERSISTENT: at most one workgroup per CU,
// whatever the contig's size.
//
// THE KERNEL'S FOOTPRINT ON A CU (measured: profiles/r06_seed_footprint.txt).  The kernel issues VALU in 20 % of its cycles and waits for
// memory in 54 %, so what it leaves FREE on a CU -- for the DP workgroups and fused passes of the other contexts -- is worth more than what that costs it:
//  * a workgroup is SEED_WPW = 8 INDEPENDENT waves, each with its own SeedLds and its own tickets, and asks for more than half a CU's LDS (SEED_WG_LDS), so exactly ONE
//    workgroup fits a CU and a launch of n_cus workgroups lands on EVERY CU (the dispatcher fills a CU before it moves on);
//  * the register budget is 96 VGPRs per wave (SEED_MIN_WAVES = 5; the LDS is a launch parameter because with static LDS the compiler knows that the LDS holds the kernel
//    at three waves per SIMD and spends the registers that leaves, whatever the launch bound says: 149).
// A CU that runs the seed kernel keeps 58 KB of LDS and ~320 VGPRs per SIMD lane free.
#define SEED_TICKET 16
#ifndef SEED_WPW
#define SEED_WPW (SEED_LDS_DIET ? 11 : 8)      // waves (= chunks in flight) per workgroup = per CU (11: what fits the same LDS at SEED_LDS_DIET's 9.0 KB per chunk, an experiment build; 12 before the claim bitmap)
#endif
#ifndef SEED_WG_LDS
#define SEED_WG_LDS 102400      // what a workgroup asks for, whatever its waves need: the 58 KB beside it are what the other contexts' kernels live on
#endif
static_assert(SEED_WPW > 1, "the production kernel is one workgroup of several independent waves per CU");
static_assert(SEED_WG_LDS > 160 * 1024 / 2 && SEED_WG_LDS <= 160 * 1024, "a workgroup's LDS: more than half a CU's, so that two never share one");
// (the accounting instance, COUNT: a one-wave workgroup that walks everything the reference's way, with a per-start Occ-block array of 20 KB)
template <bool COUNT, bool E16>
__global__ void __launch_bounds__(SEED_WG * (COUNT ? 1 : SEED_WPW), COUNT ? 1 : SEED_MIN_WAVES) k_seed_wg(DevIndex di, const uint8_t *__restrict__ q, i32 qlen, Params prm, u64 *cnt,
                                                      i32 *cand_s, i32 *cand_len, u64 *cand_x0, i32 *cand_freq, u32 cand_cap, u32 *cand_cnt, u32 *onpath, i32 *chunk_hits, u64 *hcnt,
                                                      u32 budget, u32 *heavy_list, i32 *chunk_base, u64 tk_base, u32 n_chunks, u32 lhop_cap)
{
	constexpr int WPW = COUNT ? 1 : SEED_WPW;
	typedef SeedLds<COUNT> Lds;
	static_assert(WPW == 1 || sizeof(Lds) * WPW <= SEED_WG_LDS, "SeedLds has outgrown the workgroup's LDS: SEED_WPW waves no longer fit SEED_WG_LDS bytes");
	static_assert(sizeof(Lds) % 4 == 0, "one SeedLds per wave, back to back");
	extern __shared__ __attribute__((aligned(16))) unsigned char seed_dyn_lds[];      // (a launch parameter: see the kernel's header)
	Lds *lds = (Lds *)seed_dyn_lds;
	Lds &L = lds[WPW == 1 ? 0 : (threadIdx.x >> 6)];
	for (;;) {
		u32 chunk = 0;
		if ((threadIdx.x & 63) == 0) chunk = (u32)(atomicAdd((unsigned long long *)&cnt[SEED_TICKET], 1ull) - tk_base);
		chunk = (u32)__builtin_amdgcn_readfirstlane((int)chunk);
		if (chunk >= n_chunks) return;
		seed_chunk<COUNT, E16, WPW>(di, q, qlen, prm, cnt, cand_s, cand_len, cand_x0, cand_freq, cand_cap, cand_cnt, onpath, chunk_hits, hcnt, budget, heavy_list, chunk_base, (int)chunk, n_chunks, lhop_cap, L);
	}
}


// Stage 1 for the whole contig, or -- c->split -- for the chunk range [rng_beg, rng_end) of it: chunks are searched
// independently (GSAlign.cpp:61-94: a thread takes 10 000-bp chunks off a counter; seeds never cross a chunk edge), so a
// long contig can be seeded by several GPUs and the hits sent to the GPU that chains it.  The
// kernels see the range as a contig of its own (pointer + length); only the select kernel needs the absolute position.
// At most GSA_SEED_SLOTS contexts of one GPU inside their seed-search kernels at a time (0 = no limit).  Contexts that are
// handed contigs of one size start together and stay in step -- four speculative kernels compete for the one resource that bounds
// them (random 32-byte sectors of HBM), then four chaining stages, which are chains of short dependent passes, leave the chip
// idle together (kernel timeline: profiles/archive/r03_timeline_multi_human.txt).  With a gate in front of the seed kernels the contexts
// fall out of step: one searches while the others chain and extend.
static std::mutex g_seed_mu; static std::condition_variable g_seed_cv; static int g_seed_busy[64];
struct SeedGate {
	int dev, slots; bool held;
	SeedGate(int d, int n) : dev(d & 63), slots(n), held(false) { if (slots > 0) { std::unique_lock<std::mutex> lk(g_seed_mu); g_seed_cv.wait(lk, [&] { return g_seed_busy[dev] < slots; }); g_seed_busy[dev]++; held = true; } }
	void release() { if (held) { { std::lock_guard<std::mutex> lk(g_seed_mu); g_seed_busy[dev]--; } g_seed_cv.notify_all(); held = false; } }
	~SeedGate() { release(); }
};

int stage1_seed(gsa_ctx *c)
{
	// GSA_SEED_CUS=n (experiment): the seed-search kernels run on a stream that may only use n of the CUs, spread evenly
#ifdef GSA_EXPERIMENTS
	static const int seed_cus = [] { const char *e = getenv("GSA_SEED_CUS"); return e ? atoi(e) : 0; }();
#else
	const int seed_cus = 0;
#endif
	if (seed_cus > 0 && !c->stream_seed) {
		hipDeviceProp_t pr; GSA_CHECK(c, hipGetDeviceProperties(&pr, c->device));
		const int ncu = pr.multiProcessorCount;
		std::vector<uint32_t> mask((size_t)(ncu + 31) / 32, 0u);
		for (int i = 0; i < ncu; i++) if ((long long)(i + 1) * seed_cus / ncu != (long long)i * seed_cus / ncu) mask[(size_t)i >> 5] |= 1u << (i & 31);
		GSA_CHECK(c, hipExtStreamCreateWithCUMask(&c->stream_seed, (uint32_t)mask.size(), mask.data()));
		GSA_CHECK(c, hipEventCreateWithFlags(&c->ev_seed_fork, hipEventDisableTiming));
	}
	hipStream_t st = c->stream;
	if (c->stream_seed) {      // (everything in front of the search on the main stream -- the contig's upload -- first; the host waits for the search itself)
		GSA_CHECK(c, hipEventRecord(c->ev_seed_fork, c->stream)); GSA_CHECK(c, hipStreamWaitEvent(c->stream_seed, c->ev_seed_fork, 0));
		st = c->stream_seed;
	}
	const bool split = c->split;
	const i64 all_chunks = ((i64)c->qlen + GSA_CHUNK - 1) / GSA_CHUNK;
	const i64 cb = split ? c->rng_beg : 0, ce = split ? (c->rng_end < all_chunks ? c->rng_end : all_chunks) : all_chunks;
	const i32 s_off = (i32)(cb * GSA_CHUNK);
	const i32 qlen_full = c->qlen;
	const i32 qlen = ce > cb ? (i32)(((i64)ce * GSA_CHUNK < (i64)qlen_full ? (i64)ce * GSA_CHUNK : (i64)qlen_full) - s_off) : 0;
	const uint8_t *d_q = c->q_dev + s_off;
	c->n_seeds = 0; c->n_groups = 0;
	if (qlen <= 0) return split ? prepare_pd_bitmap(c, 0) : GSA_OK;
	const i64 n_chunks = ((i64)qlen + GSA_CHUNK - 1) / GSA_CHUNK;
	size_t ccap = c->cand_cap_per_chunk;                // candidate slots per chunk (grows on overflow)
	if (!dev_ensure<u32>(c, c->d_onpath, (size_t)n_chunks * PATH_WORDS) || !dev_ensure<i32>(c, c->d_chunk_hits, (size_t)n_chunks + 1) || !dev_ensure<i32>(c, c->d_chunk_base, (size_t)n_chunks + 1)) return GSA_ERR_NOMEM;
	i64 n_hits = 0;
	u64 *cnt = c->d_cnt.as<u64>();
	// Dense mode (one search per start position, k_dense_search): every chunk under -sen, otherwise only the chunks the
	// speculative kernel gives up on.  The accounting build walks everything the reference's way and takes neither path.
	// GSA_SEED_MODE: "spec" (default) = the speculative kernel, and the right-to-left sweep (k_dense_sweep) for the chunks it gives up
	// on and for every chunk under -sen; "sweep" = every chunk through the sweep; "search" = round 2's dense kernel (one search per
	// start) in place of the sweep
	const int seed_mode = c->opt.seed_mode;
	// Which kernel for what (measured, profiles/archive/r03_seed_modes.txt): the speculative kernel wins where matches are unique (the bench
	// workload: 4.4 ms per 250 Mb against 19 for the sweep over every chunk); the sweep wins where repeats with thousands of copies make
	// most chunks exceed the speculative budget (adversarial 250 Mb: 31 ms against 62 for round 2's path); one search per start wins
	// under -sen (4.2 against 16 ms per 12 Mb: matches are short, a lane's chain of 40 starts is the longer road) and for a handful
	// of handed-over chunks.  A contig whose predecessor handed more than 40 % of its chunks over skips the speculative attempt.
	const bool sweep_all = !c->prm.bSensitive && !c->count_blocks && (seed_mode == 0 || (seed_mode == 1 && c->seed_sweep_next));
	const bool dense_all = (c->prm.bSensitive || sweep_all) && !c->count_blocks;
	const u32 budget = c->count_blocks ? 0u : c->seed_budget;
	if (dense_all && ccap < GSA_CHUNK / 5 + 64) { ccap = GSA_CHUNK / 5 + 64; c->cand_cap_per_chunk = ccap; }      // one accepted start in five at most
	u64 occ_all = 0;
#ifdef GSA_EXPERIMENTS
	static const int seed_slots = [] { const char *e = getenv("GSA_SEED_SLOTS"); return e ? atoi(e) : 0; }();
#else
	const int seed_slots = 0;
#endif
	SeedGate gate(c->device, (c->profiling || c->count_blocks) ? 0 : seed_slots);
	u64 contig_maxcand = 0;      // most candidates in one chunk of this contig
	for (int attempt = 0;; attempt++) {
		if (attempt == 8) return gsa_fail(c, GSA_ERR_LIMIT, "seed buffers keep overflowing");
		const size_t ctot = ccap * (size_t)n_chunks;
		if (!dev_ensure<i32>(c, c->d_cand_s, ctot) || !dev_ensure<i32>(c, c->d_cand_len, ctot) || !dev_ensure<u64>(c, c->d_cand_x0, ctot) || !dev_ensure<i32>(c, c->d_cand_freq, ctot) || !dev_ensure<u32>(c, c->d_cand_cnt, (size_t)n_chunks)) return GSA_ERR_NOMEM;
		if (!dense_all && !dev_ensure<u32>(c, c->d_heavy, (size_t)n_chunks)) return GSA_ERR_NOMEM;
		// (the counters were left at zero by the previous contig's last workgroup; chunk_hits[n_chunks] = 0 is written by chunk 0)
		if (c->profiling || c->prof_seed) hipEventRecord(c->ev[0], st);
		u64 hits = 0, maxcand = 0, n_heavy = dense_all ? (u64)n_chunks : 0;
		occ_all = 0;
		if (!dense_all) {
#define GSA_SEED_ARGS c->di, d_q, qlen, c->prm, cnt, c->d_cand_s.as<i32>(), c->d_cand_len.as<i32>(), c->d_cand_x0.as<u64>(), c->d_cand_freq.as<i32>(), (u32)ccap, \
			c->d_cand_cnt.as<u32>(), c->d_onpath.as<u32>(), c->d_chunk_hits.as<i32>(), c->h_cnt, budget, c->d_heavy.as<u32>(), c->d_chunk_base.as<i32>()
			// (persistent launch: ONE workgroup of SEED_WPW independent waves per CU -- its LDS is more than half a CU's, so the dispatcher cannot stack two -- every wave
			//  draws chunk after chunk from the ticket counter.  A short contig: as many workgroups as its chunks fill.  The accounting instance: one wave per workgroup, a plain grid)
			const size_t dl_count = sizeof(SeedLds<true>);
			size_t dl = sizeof(SeedLds<false>) * SEED_WPW; if (dl < SEED_WG_LDS) dl = SEED_WG_LDS;      // (the same footprint whatever the waves need: k_seed_wg asserts that they fit)
			static_assert(sizeof(SeedLds<true>) <= SEED_WG_LDS, "the accounting instance asks for less LDS than the production one");
			if (!c->seed_lds_checked) {      // (once per context: a launch the device rejects would leave the host waiting on counters nobody writes)
				hipDeviceProp_t pr; GSA_CHECK(c, hipGetDeviceProperties(&pr, c->device)); c->n_cus = pr.multiProcessorCount;
				if (pr.sharedMemPerBlock < dl) return gsa_fail(c, GSA_ERR_LIMIT, "the seed kernel needs " + std::to_string(dl) + " bytes of LDS per workgroup, this device allows " + std::to_string(pr.sharedMemPerBlock));
				c->seed_lds_checked = true;
			}
			const int wpw = c->count_blocks ? 1 : SEED_WPW;
			unsigned grid = (unsigned)((n_chunks + wpw - 1) / wpw);
			if (!c->count_blocks && (i64)c->n_cus < (i64)grid) grid = (unsigned)c->n_cus;
			const u64 tk_base = c->seed_ticket; c->seed_ticket += (u64)n_chunks + (u64)grid * (u64)wpw;      // (every wave's last draw is the one that fails)
			const u32 lhop_cap = c->opt.seed_lhop > 0 && c->opt.seed_lhop < LHOP_N ? (u32)c->opt.seed_lhop : (u32)LHOP_N;
			if (c->count_blocks) hipLaunchKernelGGL((k_seed_wg<true, false>), dim3(grid), dim3(SEED_WG), dl_count, st, GSA_SEED_ARGS, tk_base, (u32)n_chunks, lhop_cap);
			else if (c->di.kmer_e16) hipLaunchKernelGGL((k_seed_wg<false, true>), dim3(grid), dim3(SEED_WG * SEED_WPW), dl, st, GSA_SEED_ARGS, tk_base, (u32)n_chunks, lhop_cap);
			else hipLaunchKernelGGL((k_seed_wg<false, false>), dim3(grid), dim3(SEED_WG * SEED_WPW), dl, st, GSA_SEED_ARGS, tk_base, (u32)n_chunks, lhop_cap);
#undef GSA_SEED_ARGS
			GSA_CHECK(c, hipGetLastError());
			if (c->profiling || c->prof_seed) hipEventRecord(c->ev[1], st);
			// (the counters are in pinned memory when the seed kernel is done; the host waits for that, not for the scan of the
			//  per-chunk hit counts behind it)
			GSA_CHECK(c, hipEventRecord(c->ev[21], st));      // (the exclusive prefix of the per-chunk hit counts is left by the kernel's last workgroup)
			GSA_CHECK(c, hipEventSynchronize(c->ev[21]));
			hits = c->h_cnt[CNT_HITS]; maxcand = c->h_cnt[CNT_CAND]; n_heavy = c->h_cnt[CNT_HEAVY]; occ_all = c->h_cnt[CNT_OCCBLK_ALL];
			c->dbg[0] = c->h_cnt[11]; c->dbg[1] = n_heavy; c->dbg[2] = c->h_cnt[13]; c->dbg[3] = c->h_cnt[14]; c->dbg[4] = c->h_cnt[15]; c->dbg[5] = c->h_cnt[7];
			c->counters[0] = c->h_cnt[CNT_OCCBLK];
			if (seed_mode == 1) {
				// re-decided by every contig that goes through the speculative kernel.  A look that only confirms the sweep doubles the distance to
				// the next one (8, 16, 32, 64 contigs: the speculative attempt costs a repeat-rich 250 Mb contig 4.9 ms on top of its 12)
				c->seed_sweep_next = n_heavy * 5 > (u64)n_chunks * 2;
				c->seed_sweep_period = (c->seed_sweep_next && c->seed_sweep_probe) ? (c->seed_sweep_period < 64 ? c->seed_sweep_period * 2 : 64) : 8;
				c->seed_sweep_probe = false;
			}
		}
		if (n_heavy > 0) { if (int rcd = stage1_dense(c, st, d_q, qlen, n_chunks, n_heavy, dense_all, sweep_all, ccap, hits, maxcand, occ_all)) return rcd; }
		if (hits >= (1ull << 31) - 2) return gsa_fail(c, GSA_ERR_LIMIT, "more than 2^31 seeds in one contig");
		if (maxcand > ccap) { ccap = (size_t)maxcand + 256; c->cand_cap_per_chunk = ccap; continue; }
		n_hits = (i64)hits; contig_maxcand = maxcand;
		break;
	}
	gate.release();
	return stage1_select(c, n_chunks, n_hits, ccap, contig_maxcand, s_off, occ_all);
}

// ---------------------------------------------------------------------------
// leaf operator: BWT_Search for explicit windows (gsa_bwt_search_batch)
// ---------------------------------------------------------------------------
__global__ void k_search_batch(DevIndex di, const uint8_t *__restrict__ q, Params prm, i32 n, const i32 *start, const i32 *stop,
                               i32 *out_len, i32 *out_freq, i64 *out_loc)
{
	i32 i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	FmIntv ik; u32 blocks = 0, steps = 0;
	int len = fm_search(di, q, start[i], stop[i], ik, blocks);
	out_len[i] = len;
	int f = 0;
	if (len >= prm.MinSeedLength && ik.x2 <= GSA_MAX_SEED_FREQ) {
		f = (int)ik.x2;
		// even hits: the reference's LF walk on the sampled SA; odd hits: the dense SA (both must agree with bwt_sa)
		for (int h = 0; h < f; h++) out_loc[(i64)i * GSA_MAX_SEED_FREQ + h] = (h & 1) ? (i64)fm_locate(di, ik.x0 + h) : (i64)fm_locate_walk(di, ik.x0 + h, steps);
	}
	out_freq[i] = f;
}

extern "C" int gsa_bwt_search_batch(gsa_ctx *c, int32_t n, const int32_t *start, const int32_t *stop, int32_t *out_len, int32_t *out_freq, int64_t *out_loc)
{
	if (!c || n < 0) return GSA_ERR_ARG;
	if (c->qlen <= 0) return gsa_fail(c, GSA_ERR_STATE, "gsa_set_query first");
	if (n == 0) return GSA_OK;
	for (int i = 0; i < n; i++) if (start[i] < 0 || start[i] >= c->qlen || stop[i] > c->qlen || stop[i] <= start[i]) return gsa_fail(c, GSA_ERR_ARG, "window out of range");
	hipStream_t st = c->stream;
	i32 *d_start = dev_ensure<i32>(c, c->leaf[0], (size_t)n), *d_stop = dev_ensure<i32>(c, c->leaf[1], (size_t)n), *d_len = dev_ensure<i32>(c, c->leaf[2], (size_t)n), *d_freq = dev_ensure<i32>(c, c->leaf[3], (size_t)n);
	i64 *d_loc = dev_ensure<i64>(c, c->leaf[4], (size_t)n * GSA_MAX_SEED_FREQ);
	if (!d_start || !d_stop || !d_len || !d_freq || !d_loc) return GSA_ERR_NOMEM;
	GSA_CHECK(c, hipMemcpyAsync(d_start, start, n * 4, hipMemcpyHostToDevice, st));
	GSA_CHECK(c, hipMemcpyAsync(d_stop, stop, n * 4, hipMemcpyHostToDevice, st));
	hipLaunchKernelGGL(k_search_batch, dim3(grid_for(n, 64)), dim3(64), 0, st, c->di, c->q_dev, c->prm, n, d_start, d_stop, d_len, d_freq, d_loc);
	GSA_CHECK(c, hipMemcpyAsync(out_len, d_len, n * 4, hipMemcpyDeviceToHost, st));
	GSA_CHECK(c, hipMemcpyAsync(out_freq, d_freq, n * 4, hipMemcpyDeviceToHost, st));
	GSA_CHECK(c, hipMemcpyAsync(out_loc, d_loc, (size_t)n * GSA_MAX_SEED_FREQ * 8, hipMemcpyDeviceToHost, st));
	GSA_CHECK(c, hipStreamSynchronize(st));
	return GSA_OK;
}
