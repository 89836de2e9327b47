// gsalign_amd/csrc/k_seed_dense.hip -- stage 1, the dense fallback of the seed search: next(s) for EVERY start of a chunk (one search per
// start, or the right-to-left sweep), then the reference's chain over them.  For every chunk under -sen and for the chunks the speculative
// kernel (k_seed.hip) gives up on.
#include "gsa_ctx.h"
#include "gsa_fm.h"
#include "gsa_scan.h"
#include "gsa_seed.h"

// ---------------------------------------------------------------------------
// Dense mode: BWT_Search from EVERY start position of a chunk, one lane per start, then the reference's chain
// (IdentifyLocalMEM, GSAlign.cpp:61-94) by pointer jumping over next(s).  next(s) is a pure function of s, so this is
// exact; it does up to 10 000 searches per chunk where the speculative kernel above does a few hundred, so it is used
// where nearly every start is on the chain anyway or the chain cannot be guessed:
//   * -sen (stride 5 after a seed: walks that start on different residues mod 5 only merge at the next mismatch, so the
//     true entry of every sub-range depends on its predecessor -- 127 resolver rounds per chunk were measured);
//   * chunks the speculative kernel gave up on (tandem arrays with more than MaxSeedFreq copies: every start is searched
//     for ~100 bases, rejected, and followed by start+1 -- 46 ms on one workgroup for a 6-kb array).
// Same search ladder as above: presence bitmap -> k-mer table -> (Occ steps until one row is left) -> dense SA ->
// 64-base text windows.  Consecutive lanes hold consecutive starts, so a wavefront's searches end at the same mismatch.
// ---------------------------------------------------------------------------
#define DENSE_TPB 256
// SPAN = starts per workgroup: 512 (two per lane) when every chunk is dense (-sen), 256 for the few chunks the speculative
// kernel gave up on (their searches are ~100 dependent Occ steps each: one per lane halves the latency of that detour)
#define DENSE_WGS(SPAN) ((GSA_CHUNK + (SPAN) - 1) / (SPAN))
template <bool E16, int DENSE_SPAN>
__global__ void __launch_bounds__(DENSE_TPB) k_dense_search(DevIndex di, const uint8_t *__restrict__ q, i32 qlen, Params prm, const u32 *__restrict__ chunk_list,
                                                              u32 *dn_lf, u64 *dn_x0, u64 *cnt)
{
	__shared__ u32 qp[QP_WORDS], qn[QN_WORDS];
	const u32 slot = blockIdx.x / DENSE_WGS(DENSE_SPAN), part = blockIdx.x % DENSE_WGS(DENSE_SPAN);
	const u32 chunk = chunk_list ? chunk_list[slot] : slot;
	const int j = threadIdx.x;
	const i64 c0 = (i64)chunk * GSA_CHUNK;
	const int clen = (int)((i64)qlen - c0 < GSA_CHUNK ? (i64)qlen - c0 : GSA_CHUNK);
	const int span0 = (int)part * DENSE_SPAN, span1 = span0 + DENSE_SPAN < clen ? span0 + DENSE_SPAN : clen;
	if (span0 >= clen) return;
	// stage the chunk from the first start of this workgroup to its end (a match may run that far)
	for (int g = (span0 >> 5) + j; g < QN_WORDS; g += DENSE_TPB) {
		u32 w0 = 0, w1 = 0, wn = 0;
		const int p0 = g << 5;
		if (p0 < clen) {
			stage32(q + c0 + p0, p0, clen, w0, w1, wn);
		}
		if (2 * g < QP_WORDS) qp[2 * g] = w0;
		if (2 * g + 1 < QP_WORDS) qp[2 * g + 1] = w1;
		qn[g] = wn;
	}
	__syncthreads();
	u32 *lf = dn_lf + (size_t)slot * GSA_CHUNK; u64 *x0o = dn_x0 + (size_t)slot * GSA_CHUNK;
	int nextp = span0 + j;                                  // this lane's starts: nextp, nextp + DENSE_TPB
	int s = 0, pos = 0, mode = M_ADV; u32 kid = 0, pid = 0, pext = 0, blk = 0, all_blocks = 0;
	FmIntv ik = {0, 0, 0}; i64 tp = 0;
	const int L = prm.MinSeedLength < 32 ? prm.MinSeedLength : 32;
	while (!__all(mode == M_DONE)) {
		// ---- request phase: one pending request per lane, all lanes issue together ----
		u64 kk = 0, ll = 0; bool kn = true, ln = true;
		if (mode == M_FM) {
			const u64 k = ik.x1 - 1, l = ik.x1 - 1 + ik.x2;
			kn = (k == (u64)-1); ln = (l == (u64)-1);
			kk = kn ? 0 : k - (k >= di.primary); ll = ln ? 0 : l - (l >= di.primary);
		}
		const FmBlock bk = fm_load(di, kk >> 6), bl = fm_load(di, ll >> 6);
		struct __attribute__((packed, aligned(4))) W5 { u32 a, b, c, d, e; };
		const W5 w5 = *(const W5 *)(di.ref2 + (mode == M_TEXT ? (tp >> 4) : 0));
		ulonglong2 e0 = {0, 0}, e1 = {0, 0};
		if (E16) {
			const uint4 e = ((const uint4 *)(di.kmer ? di.kmer : (const u64 *)di.bwt))[mode == M_KMER ? kid : 0];
			e0.x = e.x; e0.y = e.y; e1.x = e.z; e1.y = e.w;
		} else {
			const ulonglong2 *pe = (const ulonglong2 *)((di.kmer ? di.kmer : (const u64 *)di.bwt) + (mode == M_KMER ? ((size_t)kid << 2) : 0));
			e0 = pe[0]; e1 = pe[1];
		}
		// the short table: for a start whose kmer_k-mer does not occur (its match ends before kmer_k bases) -- the common case
		// under -sen, where a match of 10..14 bases is a seed -- the interval after kmer_lo_k bases, instead of walking them
		ulonglong2 l0 = {0, 0}, l1 = {0, 0};
		if (di.kmer_lo) {
			if (E16) { const uint4 e = ((const uint4 *)di.kmer_lo)[mode == M_KLO ? kid : 0]; l0.x = e.x; l0.y = e.y; l1.x = e.z; l1.y = e.w; }
			else { const ulonglong2 *pe = (const ulonglong2 *)(di.kmer_lo + (mode == M_KLO ? ((size_t)kid << 2) : 0)); l0 = pe[0]; l1 = pe[1]; }
		}
		// (one start per lane here: role 0 of the group that starts at s -- dword pid of the grouped presence table, bit pext)
		const u32 pw = di.pres ? di.pres[mode == M_KMER ? pid : 0] : ~0u;
		const u64 sav = fm_locate(di, mode == M_LOC ? ik.x0 : 1);
		// ---- consume phase ----
		bool ended = false;
		if (mode == M_KMER) {
			if (!((pw >> pext) & 1u)) { ended = true; pos = s; ik.x2 = 0; }      // the first MinSeedLength bases do not occur: no seed here
			else {
				const bool hit = e1.x != 0;         // absent k-mer: the match is shorter than k
				if (hit) { ik.x0 = e0.x; ik.x1 = e0.y; ik.x2 = e1.x; pos = s + di.kmer_k; }
				mode = M_FM;                        // (no short table: walk it base by base from the first base)
				if (hit && ik.x2 == 1) { tp = (i64)(e1.y - 1) + di.kmer_k; mode = M_TEXT; }
				if (!hit && di.kmer_lo) { kid = kid & ((1u << (2 * di.kmer_lo_k)) - 1); mode = M_KLO; }      // (the start passed the N / length tests for kmer_k >= kmer_lo_k bases)
			}
		} else if (mode == M_KLO) {
			const bool hit = l1.x != 0;
			if (hit) { ik.x0 = l0.x; ik.x1 = l0.y; ik.x2 = l1.x; pos = s + di.kmer_lo_k; }
			mode = M_FM;
			if (hit && ik.x2 == 1) { tp = (i64)(l1.y - 1) + di.kmer_lo_k; mode = M_TEXT; }
		} else if (mode == M_LOC) {
			tp = (i64)sav + (pos - s); mode = M_TEXT;
		} else if (mode == M_TEXT) {
			int got = text_match32(w5.a, w5.b, w5.c, tp, (i64)di.seq_len, qp, qn, pos, clen);
			if (got == 32) got += text_match32(w5.c, w5.d, w5.e, tp + 32, (i64)di.seq_len, qp, qn, pos + 32, clen);
			pos += got; tp += got;
			ended = got < 64;
		} else if (mode == M_FM) {
			const bool can = pos < clen && !q_isn(qn, pos < clen ? pos : 0);
			const bool ok = can && fm_extend_loaded(di, ik, q_code(qp, pos < clen ? pos : 0), bk, bl, kk, ll, kn, ln, blk);
			ended = !ok;
			if (ok) { pos++; if (ik.x2 == 1) mode = M_LOC; }
		}
		if (ended) {
			const int len = pos - s;
			u32 rec = 0;
			if (len >= prm.MinSeedLength && ik.x2 <= GSA_MAX_SEED_FREQ) { rec = (u32)len | ((u32)ik.x2 << 16); x0o[s] = ik.x0; }
			lf[s] = rec;      // (the hop follows from the record: k_dense_resolve)
			all_blocks += blk;
			mode = M_ADV;
		}
		// ---- next start of this lane (starts that need no search are settled here, two per iteration) ----
		for (int step = 0; step < 2 && mode == M_ADV; step++) {
			if (nextp >= span1) { mode = M_DONE; break; }
			s = nextp; nextp += DENSE_TPB;
			const u32 nb = q_nbits32(qn, s);
			if ((nb & 1u) || s + prm.MinSeedLength > clen || (nb & (L == 32 ? ~0u : (1u << L) - 1)) != 0) { lf[s] = 0; continue; }      // ambiguous start, or MinSeedLength out of reach
			ik = fm_init(di, q_code(qp, s)); pos = s + 1; blk = 0; mode = M_FM;
			if (di.kmer_k > 1 && s + di.kmer_k <= clen && (nb & ((1u << di.kmer_k) - 1)) == 0) {
				const u64 qb = q_bits64(qp, s);
				kid = (u32)(qb & ((1ull << (2 * di.kmer_k)) - 1)); mode = M_KMER;
				{ const u32 b0 = di.pres_k ? pres4_bit(qb, di.pres_k, 0) : 0; pid = di.pres_k ? pres4_line(qb, di.pres_k) * 8 + (b0 >> 5) : 0; pext = b0 & 31u; }
			} else if (di.kmer_lo && s + di.kmer_lo_k <= clen && (nb & ((1u << di.kmer_lo_k) - 1)) == 0) {
				kid = (u32)(q_bits64(qp, s) & ((1ull << (2 * di.kmer_lo_k)) - 1)); mode = M_KLO;      // (too close to the chunk end or an N for the long table)
			}
		}
	}
	for (int o = 32; o; o >>= 1) all_blocks += __shfl_down(all_blocks, o);
	if ((j & 63) == 0 && all_blocks) atomicAdd((unsigned long long *)&cnt[CNT_OCCBLK_ALL], (unsigned long long)all_blocks);
}

// ---------------------------------------------------------------------------
// Sweep mode (round 3): next(s) for EVERY start of a chunk like k_dense_search, but not one search per start.  Two facts about
// L(s), the length of the longest match from s (what BWT_Search computes; its interval = all occurrences of q[s .. s+L(s))):
//   (1) L(s) <= L(s+1) + 1                    (q[s+1 .. s+L(s)) occurs)
//   (2) if q[s+1 .. e) is the longest match from s+1 and q[s .. e) occurs, then L(s) = e - s      (by (1))
// So a lane that owns SWEEP_SEG consecutive starts walks them RIGHT TO LEFT: one forward search from scratch for its last start
// (presence table -> k-mer table -> Occ steps -> dense SA -> 64-base text windows, as above), then for every start to the left
// it only asks "does the match extend by one base on the left?":
//   * the match is unique (one occurrence, at text position t): it extends iff text[t-1] equals the query base, and stays
//     unique -- 32 starts per comparison of packed words (M_BACK), no index access at all;
//   * the match has several occurrences (a repeat): ONE backward extension of the bi-interval (x0, x1, x2) -- the index is
//     symmetric (forward + reverse-complement text), so prepending base c is the forward step of the reference's BWT_Search
//     (bwt_search.cpp:152-165) with x0 and x1 swapped and the complementary base (M_BFM): one Occ step per start where the
//     reference and k_dense_search walk ~L(s) steps per start -- the `freq > MaxSeedFreq` reject-and-restart regime of
//     bwt_search.cpp:177-182 costs O(L) per copy of a repeat instead of O(L^2);
//   * it does not extend: L(s) < e - s, and the lane searches forward from s from scratch (exact by definition).
// Nothing is speculated and no lane depends on another: next(s) is a pure function of s.  Same outputs as k_dense_search
// (lf / x0 per start), so k_dense_resolve and everything downstream are unchanged; a unique match found by text
// comparison has no SA row at hand, so its x0 carries the text POSITION with bit 63 set (k_seed_select takes it as located).
// ---------------------------------------------------------------------------
#define SWEEP_POSFLAG (1ull << 63)
enum { M_BFM = 7, M_BACK = 8, M_LOC2 = 9 };
enum { HV_NONE = 0, HV_UNIQ = 1, HV_MULTI = 2 };
#ifndef SWEEP_NCH
#define SWEEP_NCH 4            // chunks per workgroup (3.75 KB of LDS each)
#endif
#ifndef SWEEP_TPB
#define SWEEP_TPB 128
#endif
template <bool E16, int NCH, int TPB>
__global__ void __launch_bounds__(TPB) k_dense_sweep(DevIndex di, const uint8_t *__restrict__ q, i32 qlen, Params prm, const u32 *__restrict__ chunk_list, u32 n_slots,
                                                     u32 *dn_lf, u64 *dn_x0, u64 *cnt, int seg)
{
	// seg = starts per segment; long segments do the least work (one forward search per segment), short ones finish soonest.
	// Round 3 ran four waves per chunk with 40 starts per lane; round 4 first ONE wave per chunk with 160: inside a high-copy repeat a
	// segment costs ~150 Occ steps for its first (forward) search and one backward step per start, so 40 starts cost a lane 190
	// dependent steps and 160 cost it 310 -- a quarter of the forward searches.  But a lane in unique sequence is through with its
	// 160 starts after ~14 steps, and three lanes in four waited for the wave's repeat lanes while the kernel is bound by the
	// instructions its waves issue (tools/r4_adv_pmc.sh: 6.0 G VALU wave-instructions per 250 Mb, 318 iterations per wave).  So now
	// ONE WAVE takes NCH chunks and its lanes DRAW the segments (63 per chunk) from a counter in LDS: a lane that is through
	// takes the next one, whichever chunk it belongs to -- every lane carries its chunk (query words in LDS, record arrays) along.
	__shared__ u32 qp[NCH][QP_WORDS], qn[NCH][QN_WORDS];
	__shared__ u32 s_next;
	const int j = threadIdx.x;
	const u32 slot0 = blockIdx.x * (u32)NCH;
	const int nch = (int)(n_slots - slot0 < (u32)NCH ? n_slots - slot0 : (u32)NCH);
	const int spc = (GSA_CHUNK + seg - 1) / seg;                  // segments per chunk
	const u32 n_seg = (u32)(nch * spc);
	for (int ch = 0; ch < nch; ch++) {
		const u32 chunk = chunk_list ? chunk_list[slot0 + ch] : slot0 + ch;
		const i64 c0 = (i64)chunk * GSA_CHUNK;
		const int cl = (int)((i64)qlen - c0 < GSA_CHUNK ? (i64)qlen - c0 : GSA_CHUNK);
		for (int g = j; g < QN_WORDS; g += TPB) {
			u32 w0 = 0, w1 = 0, wn = 0;
			const int p0 = g << 5;
			if (p0 < cl) {
				stage32(q + c0 + p0, p0, cl, w0, w1, wn);
			} else wn = ~0u;
			if (2 * g < QP_WORDS) qp[ch][2 * g] = w0;
			if (2 * g + 1 < QP_WORDS) qp[ch][2 * g + 1] = w1;
			qn[ch][g] = wn;
		}
	}
	if (j == 0) s_next = 0;
	__syncthreads();
	// the lane's segment: chunk-relative starts [seg_a, cur] of the chunk whose words are qp_l / qn_l and whose records are lf / x0o
	const u32 *qp_l = qp[0], *qn_l = qn[0]; u32 *lf = dn_lf; u64 *x0o = dn_x0; int clen = 0;
	int seg_a = 0;
	int cur = -1;                                              // next start to settle; the lane draws a segment when cur < seg_a
	int s = 0, pos = 0, mode = M_ADV, have = HV_NONE, e_end = 0, prole = 0; u32 kid = 0, pid = 0, blk = 0, all_blocks = 0;
	u64 pqb = 0;
	FmIntv ik = {0, 0, 0}; i64 tp = 0, tps = 0;
	const int L = prm.MinSeedLength < 32 ? prm.MinSeedLength : 32;
	const u32 Lmask = L == 32 ? ~0u : (1u << L) - 1;
	// what is known about start S_ once its longest match [S_, S_ + LEN_) with X2_ occurrences is: the seed record (the hop follows from it)
#define SWEEP_SETTLE(S_, LEN_, X2_, X0_) \
	{ \
		u32 rec_ = 0; \
		if ((LEN_) >= prm.MinSeedLength && (X2_) <= (u64)GSA_MAX_SEED_FREQ) { rec_ = (u32)(LEN_) | ((u32)(X2_) << 16); x0o[S_] = (X0_); } \
		lf[S_] = rec_; \
	}
	while (!__all(mode == M_DONE)) {
		// ---- request phase: one pending request per lane, all lanes issue together ----
		u64 kk = 0, ll = 0; bool kn = true, ln = true;
		if (mode == M_FM || mode == M_BFM) {
			const u64 xr = mode == M_FM ? ik.x1 : ik.x0;      // forward extension counts on the reverse-strand interval, backward extension on the forward one
			const u64 k = xr - 1, l = xr - 1 + ik.x2;
			kn = (k == (u64)-1); ln = (l == (u64)-1);
			kk = kn ? 0 : k - (k >= di.primary); ll = ln ? 0 : l - (l >= di.primary);
		}
		const FmBlock bk = fm_load(di, kk >> 6), bl = fm_load(di, ll >> 6);
		struct __attribute__((packed, aligned(4))) W5 { u32 a, b, c, d, e; };
		// forward: 64 bases from tp on; backward (M_BACK): the three words that end with the base in front of the match
		const i64 bw_word = ((tps - 1) >> 4) - 2 > 0 ? ((tps - 1) >> 4) - 2 : 0;
		const W5 w5 = *(const W5 *)(di.ref2 + (mode == M_TEXT ? (tp >> 4) : (mode == M_BACK ? bw_word : 0)));
		ulonglong2 e0 = {0, 0}, e1 = {0, 0};
		if (E16) {
			const uint4 e = ((const uint4 *)(di.kmer ? di.kmer : (const u64 *)di.bwt))[mode == M_KMER ? kid : 0];
			e0.x = e.x; e0.y = e.y; e1.x = e.z; e1.y = e.w;
		} else {
			const ulonglong2 *pe = (const ulonglong2 *)((di.kmer ? di.kmer : (const u64 *)di.bwt) + (mode == M_KMER ? ((size_t)kid << 2) : 0));
			e0 = pe[0]; e1 = pe[1];
		}
		ulonglong2 l0 = {0, 0}, l1 = {0, 0};
		if (di.kmer_lo) {
			if (E16) { const uint4 e = ((const uint4 *)di.kmer_lo)[mode == M_KLO ? kid : 0]; l0.x = e.x; l0.y = e.y; l1.x = e.z; l1.y = e.w; }
			else { const ulonglong2 *pe = (const ulonglong2 *)(di.kmer_lo + (mode == M_KLO ? ((size_t)kid << 2) : 0)); l0 = pe[0]; l1 = pe[1]; }
		}
		// the line of the grouped presence table that answers for the start and up to three starts to its LEFT (pid = line, prole = role of s)
		uint4 pl0 = {~0u, ~0u, ~0u, ~0u}, pl1 = {~0u, ~0u, ~0u, ~0u};
		if (di.pres) { const uint4 *pp = (const uint4 *)di.pres + 2 * (size_t)(mode == M_KMER ? pid : 0); pl0 = pp[0]; pl1 = pp[1]; }
		const u64 sav = fm_locate(di, (mode == M_LOC || mode == M_LOC2) ? ik.x0 : 1);
		// ---- consume phase ----
		bool ended = false;
		if (mode == M_KMER) {
			// role r of the line: dword 2 r + (e >> 5), bit e & 31, e = pres4_bit(pqb, K, r) & 63 -- all four answers as a mask
			u32 pmask = 15u;
			if (di.pres) {
				const u32 e0_ = pres4_bit(pqb, di.pres_k, 0) & 63u, e1_ = pres4_bit(pqb, di.pres_k, 1) & 63u, e2_ = pres4_bit(pqb, di.pres_k, 2) & 63u, e3_ = pres4_bit(pqb, di.pres_k, 3) & 63u;
				pmask = ((((e0_ & 32u) ? pl0.y : pl0.x) >> (e0_ & 31u)) & 1u) | (((((e1_ & 32u) ? pl0.w : pl0.z) >> (e1_ & 31u)) & 1u) << 1)
				      | (((((e2_ & 32u) ? pl1.y : pl1.x) >> (e2_ & 31u)) & 1u) << 2) | (((((e3_ & 32u) ? pl1.w : pl1.z) >> (e3_ & 31u)) & 1u) << 3);
			}
			auto present = [&](int r) -> bool { return (pmask >> r) & 1u; };
			if (!present(prole)) {
				// the first MinSeedLength bases of s do not occur: no seed, nothing to extend; the same line answers for the starts to
				// the left while they pass the N / length tests (their own hop is 1 as well when they do not)
				lf[s] = 0; cur = s - 1; have = HV_NONE; mode = M_ADV;
				for (int r = prole - 1; r >= 0 && cur >= seg_a; r--) {
					const u32 nb = q_nbits32(qn_l, cur);
					if ((nb & 1u) || cur + prm.MinSeedLength > clen || (nb & Lmask) != 0) break;      // (the advance step settles those)
					if (present(r)) break;                                                            // occurs: needs its own search
					lf[cur] = 0; cur--;
				}
			} else {
				const bool hit = e1.x != 0;         // absent k-mer: the match is shorter than k
				if (hit) { ik.x0 = e0.x; ik.x1 = e0.y; ik.x2 = e1.x; pos = s + di.kmer_k; }
				mode = M_FM;
				if (hit && ik.x2 == 1) { tp = (i64)(e1.y - 1) + di.kmer_k; mode = M_TEXT; }
				if (!hit && di.kmer_lo) { kid = kid & ((1u << (2 * di.kmer_lo_k)) - 1); mode = M_KLO; }
			}
		} else if (mode == M_KLO) {
			const bool hit = l1.x != 0;
			if (hit) { ik.x0 = l0.x; ik.x1 = l0.y; ik.x2 = l1.x; pos = s + di.kmer_lo_k; }
			mode = M_FM;
			if (hit && ik.x2 == 1) { tp = (i64)(l1.y - 1) + di.kmer_lo_k; mode = M_TEXT; }
		} else if (mode == M_LOC) {
			tp = (i64)sav + (pos - s); mode = M_TEXT;
		} else if (mode == M_TEXT) {
			int got = text_match32(w5.a, w5.b, w5.c, tp, (i64)di.seq_len, qp_l, qn_l, pos, clen);
			if (got == 32) got += text_match32(w5.c, w5.d, w5.e, tp + 32, (i64)di.seq_len, qp_l, qn_l, pos + 32, clen);
			pos += got; tp += got;
			ended = got < 64;
		} else if (mode == M_FM || mode == M_BFM) {
			// one Occ step for both directions (a wave has lanes in either most of the time: the step is the heaviest block of the loop).
			// Forward: append q[pos] to [s, pos).  Backward: prepend q[cur] to the match [cur + 1, e_end) -- the reference's forward step
			// on the mirrored bi-interval with the complementary base
			const bool bw = mode == M_BFM;
			const int qi = bw ? cur : (pos < clen ? pos : 0);
			const bool can = bw || (pos < clen && !q_isn(qn_l, qi));
			const int code = q_code(qp_l, qi);
			FmIntv m = { bw ? ik.x1 : ik.x0, bw ? ik.x0 : ik.x1, ik.x2 };
			const bool ok = can && fm_extend_loaded(di, m, bw ? 3 - code : code, bk, bl, kk, ll, kn, ln, blk);
			if (ok) { ik.x0 = bw ? m.x1 : m.x0; ik.x1 = bw ? m.x0 : m.x1; ik.x2 = m.x2; }
			if (!bw) {
				ended = !ok;
				if (ok) { pos++; if (ik.x2 == 1) mode = M_LOC; }
			} else {
				all_blocks += blk; blk = 0;
				if (ok) {
					SWEEP_SETTLE(cur, e_end - cur, ik.x2, ik.x0)
					cur--;
					mode = ik.x2 == 1 ? M_LOC2 : M_ADV;       // one occurrence left: from here on the text itself answers
				} else { have = HV_NONE; mode = M_ADV; }      // (L(cur) < e_end - cur: search forward from cur)
			}
		} else if (mode == M_LOC2) {
			tps = (i64)sav; have = HV_UNIQ; mode = M_ADV;      // text position of start cur + 1
		} else if (mode == M_BACK) {
			// the match [cur + 1, e_end) sits once in the text, at tps: start cur - t extends it iff the t + 1 bases in front agree
			int n = cur - seg_a + 1; if (n > 32) n = 32; if ((i64)n > tps) n = (int)tps;
			int nbk = 0;
			if (n > 0) {
				const int off = (int)(tps - n - (bw_word << 4));                 // first compared text base inside the three words (0 .. 47)
				const u64 lo64 = (u64)w5.a | ((u64)w5.b << 32), hi64 = (u64)w5.c;
				const int sh = off * 2;
				const u64 T = sh == 0 ? lo64 : (sh < 64 ? (lo64 >> sh) | (hi64 << (64 - sh)) : (hi64 >> (sh - 64)));
				const u64 Q = q_bits64(qp_l, cur - n + 1);
				const u64 msk = n == 32 ? ~0ull : ((1ull << (2 * n)) - 1);
				const u64 d = (Q ^ T) & msk;
				const u64 dm = (d | (d >> 1)) & 0x5555555555555555ull;
				const u32 nm = q_nbits32(qn_l, cur - n + 1) & (n == 32 ? ~0u : ((1u << n) - 1));
				const int im = dm ? (63 - __clzll((long long)dm)) >> 1 : -1, in_ = nm ? 31 - __clz((int)nm) : -1;
				nbk = n - 1 - (im > in_ ? im : in_);
			}
			// the nbk starts [cur - nbk + 1, cur] are settled at once: start a + i matches [a + i, e_end) once, at text position tps - nbk + i.
			// Four starts per store (dword-aligned 16-byte stores: the records of a run are consecutive) -- a lane in unique sequence
			// settles 32 starts per iteration, and one scalar store per array and start was most of what the kernel asked of the L2
			{
				const int a = cur - nbk + 1;
				struct __attribute__((packed, aligned(4))) R4 { u32 v[4]; };
				struct __attribute__((packed, aligned(8))) X4 { u64 v[4]; };
				int i = 0;
				for (; i + 4 <= nbk; i += 4) {
					R4 r; X4 x;
#pragma unroll
					for (int e = 0; e < 4; e++) {
						const int len_ = e_end - (a + i + e);
						r.v[e] = len_ >= prm.MinSeedLength ? (u32)len_ | (1u << 16) : 0u;      // (SWEEP_SETTLE with one occurrence; -sen does not come here)
						x.v[e] = SWEEP_POSFLAG | (u64)(tps - nbk + i + e);
					}
					*(R4 *)(lf + a + i) = r; *(X4 *)(x0o + a + i) = x;
				}
				for (; i < nbk; i++) { const int st = a + i; SWEEP_SETTLE(st, e_end - st, 1ull, SWEEP_POSFLAG | (u64)(tps - nbk + i)) }
			}
			cur -= nbk; tps -= nbk;
			if (nbk < n || n <= 0) have = HV_NONE;                                  // stopped by a mismatch, an N or the start of the text
			mode = M_ADV;
		}
		if (ended) {
			// the forward search from s is through: [s, pos) with ik.x2 occurrences (ik.x0 = first row)
			const int len = pos - s;
			SWEEP_SETTLE(s, len, ik.x2, ik.x0)
			all_blocks += blk; blk = 0;
			cur = s - 1; e_end = pos;
			if (mode == M_TEXT) { have = HV_UNIQ; tps = tp - (i64)len; }            // (tp is the text position of pos)
			else have = (len >= 1 && ik.x2 >= 1) ? HV_MULTI : HV_NONE;
			mode = M_ADV;
		}
		// ---- what to do about start cur ----
		for (int step = 0; step < 3 && mode == M_ADV; step++) {
			if (cur < seg_a) {
				// through with the segment: the next one of the wave's chunks (LDS counter; M_DONE when they are all handed out)
				const u32 id = atomicAdd(&s_next, 1u);
				if (id >= n_seg) { mode = M_DONE; break; }
				const int ch = (int)id / spc, sg = (int)id - ch * spc;
				const u32 chunk = chunk_list ? chunk_list[slot0 + ch] : slot0 + ch;
				const i64 c0 = (i64)chunk * GSA_CHUNK;
				clen = (int)((i64)qlen - c0 < GSA_CHUNK ? (i64)qlen - c0 : GSA_CHUNK);
				qp_l = qp[ch]; qn_l = qn[ch]; lf = dn_lf + (size_t)(slot0 + ch) * GSA_CHUNK; x0o = dn_x0 + (size_t)(slot0 + ch) * GSA_CHUNK;
				seg_a = sg * seg; cur = (seg_a + seg < clen ? seg_a + seg : clen) - 1; have = HV_NONE;
				continue;
			}
			const u32 nb = q_nbits32(qn_l, cur);
			if (nb & 1u) { lf[cur] = 0; have = HV_NONE; cur--; continue; }      // ambiguous base: no search from here, nothing extends over it
			if (have == HV_UNIQ) { mode = M_BACK; break; }
			if (have == HV_MULTI) { mode = M_BFM; break; }
			if (cur + prm.MinSeedLength > clen || (nb & Lmask) != 0) { lf[cur] = 0; cur--; continue; }      // MinSeedLength out of reach
			s = cur; ik = fm_init(di, q_code(qp_l, s)); pos = s + 1; blk = 0; mode = M_FM;
			if (di.kmer_k > 1 && s + di.kmer_k <= clen && (nb & ((1u << di.kmer_k) - 1)) == 0) {
				kid = (u32)(q_bits64(qp_l, s) & ((1ull << (2 * di.kmer_k)) - 1)); mode = M_KMER;
				// presence: the group that starts three bases to the left (as far as the chunk goes), s in its last role
				prole = s >= 3 ? 3 : s;
				pqb = q_bits64(qp_l, s - prole);
				pid = di.pres_k ? pres4_line(pqb, di.pres_k) : 0;
			} else if (di.kmer_lo && s + di.kmer_lo_k <= clen && (nb & ((1u << di.kmer_lo_k) - 1)) == 0) {
				kid = (u32)(q_bits64(qp_l, s) & ((1ull << (2 * di.kmer_lo_k)) - 1)); mode = M_KLO;
			}
		}
	}
#undef SWEEP_SETTLE
	for (int o = 32; o; o >>= 1) all_blocks += __shfl_down(all_blocks, o);
	if ((j & 63) == 0 && all_blocks) atomicAdd((unsigned long long *)&cnt[CNT_OCCBLK_ALL], (unsigned long long)all_blocks);
}

// The chain of a dense chunk: orbit of 0 under p -> next(p) (from the start's record), then the accepted on-chain matches go to
// the chunk's candidate segment in the layout k_seed_wg leaves (so everything downstream is the same).  Round 3 marked the orbit by
// pointer doubling over all 10 000 positions (14 rounds: 2.8 ms per 250 Mb of dense chunks, a fifth of their seed stage).  next() only
// moves forward, so the chunk is cut into 256 blocks of 40 positions, one per thread:
//   1. every thread resolves its block from right to left: ex[p] = where the path through p LEAVES the block (40 dependent LDS reads);
//   2. one thread follows 0 -> ex[0] -> ex[ex[0]] ... (at most one step per block) and notes where the path enters each block;
//   3. every thread whose block the path enters walks it inside the block and marks the positions.
#define RS_B 40                 // positions per thread
#define RS_XS 42                // block stride of ex[] (u16; 21 dwords: odd, so the threads' blocks fall into different banks)
#define RS_HS 44                // block stride of hopb[] (u8; 11 dwords)
static_assert(256 * RS_B >= GSA_CHUNK, "one block per thread");
__global__ void __launch_bounds__(256) k_dense_resolve(const u32 *__restrict__ chunk_list, u32 n_total_chunks, i32 qlen, int sen, const u32 *__restrict__ dn_lf,
                                                        const u64 *__restrict__ dn_x0, u64 *cnt, i32 *cand_s, i32 *cand_len, u64 *cand_x0, i32 *cand_freq, u32 cand_cap, u32 *cand_cnt,
                                                        u32 *onpath, i32 *chunk_hits, u64 *hcnt, i32 *chunk_base)
{
	__shared__ uint16_t ex[256 * RS_XS];        // first position outside p's block on the path through p (0xffff: outside the chunk)
	__shared__ uint8_t hopb[256 * RS_HS];       // next(p) - p where that stays inside p's block, else 0
	__shared__ uint16_t s_entry[256];           // where the path from 0 enters the block (0xffff: it jumps over it)
	__shared__ u32 bits[PATH_WORDS];
	__shared__ u32 s_n, s_hits;
	__shared__ int s_last;
	const u32 slot = blockIdx.x, chunk = chunk_list ? chunk_list[slot] : slot;
	const int j = threadIdx.x;
	const i64 c0 = (i64)chunk * GSA_CHUNK;
	const int clen = (int)((i64)qlen - c0 < GSA_CHUNK ? (i64)qlen - c0 : GSA_CHUNK);
	const u32 *lf = dn_lf + (size_t)slot * GSA_CHUNK; const u64 *x0 = dn_x0 + (size_t)slot * GSA_CHUNK;
	// next(p): behind an accepted match (five bases on with -sen), else the next base -- the record says which (GSAlign.cpp:61-94)
	for (int p = j; p < clen; p += 256) {
		const u32 rec = lf[p];
		const int hop = rec ? (sen ? 5 : (int)(rec & 0xffffu) + 1) : 1, t = p + hop;
		const int b = p / RS_B, i = p - b * RS_B, bend = (b + 1) * RS_B < clen ? (b + 1) * RS_B : clen;
		ex[b * RS_XS + i] = (uint16_t)(t < clen ? t : 0xffff);
		hopb[b * RS_HS + i] = (uint8_t)(t < bend ? hop : 0);
	}
	for (int w = j; w < PATH_WORDS; w += 256) bits[w] = 0u;
	s_entry[j] = 0xffff;
	if (j == 0) { s_n = 0; s_hits = 0; }
	__syncthreads();
	{
		const int n = clen - j * RS_B < RS_B ? clen - j * RS_B : RS_B;      // (<= 0: the chunk ends in front of this block)
		for (int i = n - 1; i >= 0; i--) { const int h = hopb[j * RS_HS + i]; if (h) ex[j * RS_XS + i] = ex[j * RS_XS + i + h]; }
	}
	__syncthreads();
	if (j == 0) for (int e = 0; e != 0xffff;) { const int b = e / RS_B; s_entry[b] = (uint16_t)e; e = ex[b * RS_XS + (e - b * RS_B)]; }
	__syncthreads();
	if (s_entry[j] != 0xffff)
		for (int i = (int)s_entry[j] - j * RS_B;;) {
			const int p = j * RS_B + i;
			atomicOr(&bits[p >> 5], 1u << (p & 31));
			const int h = hopb[j * RS_HS + i];
			if (!h) break;
			i += h;
		}
	__syncthreads();
	const size_t cbase = (size_t)chunk * cand_cap;
	u32 h = 0;
	for (int p = j; p < clen; p += 256) {
		if (!((bits[p >> 5] >> (p & 31)) & 1u)) continue;
		const u32 rec = lf[p];
		if (!rec) continue;
		const u32 k = atomicAdd(&s_n, 1u);
		if (k < cand_cap) { cand_s[cbase + k] = (i32)(c0 + p); cand_len[cbase + k] = (i32)(rec & 0xffffu); cand_x0[cbase + k] = x0[p]; cand_freq[cbase + k] = (i32)(rec >> 16); h += rec >> 16; }
	}
	for (int o = 32; o; o >>= 1) h += __shfl_down(h, o);
	if ((j & 63) == 0 && h) atomicAdd(&s_hits, h);
	for (int w = j; w < PATH_WORDS; w += 256) onpath[(size_t)chunk * PATH_WORDS + w] = bits[w];
	__syncthreads();
	if (j == 0) {
		cand_cnt[chunk] = s_n < cand_cap ? s_n : cand_cap; lb_pub(&chunk_hits[chunk], (i32)s_hits); if (slot == 0) lb_pub(&chunk_hits[n_total_chunks], 0);
		atomicMax((unsigned long long *)&cnt[CNT_CAND], (unsigned long long)s_n);
		if (s_hits) atomicAdd((unsigned long long *)&cnt[CNT_HITS], (unsigned long long)s_hits);
		asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");      // (counters are device atomics; an agent-scope fence is an L2 write-back per workgroup here)
		s_last = atomicAdd((unsigned long long *)&cnt[CNT_DONE], 1ull) == (unsigned long long)gridDim.x - 1 ? 1 : 0;
	}
	__syncthreads();
	// the last workgroup puts the counters into pinned memory and leaves them at zero (as k_seed_wg does)
	if (s_last && j < 16) {
		hcnt[j] = j == CNT_DONE ? 0 : __hip_atomic_load(&cnt[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		cnt[j] = 0;
	}
	if (s_last) wg_exscan_hits<256>(chunk_hits, chunk_base, (int)n_total_chunks + 1);      // (every chunk's count: those of the speculative kernel too)
}

// The dense kernels over n_heavy chunks -- every chunk of the range (dense_all) or the ones the speculative kernel listed in d_heavy -- and their resolve; waits
// for them and adds their counters to the caller's.  Which kernel for what: see stage1_seed (k_seed.hip).
int stage1_dense(gsa_ctx *c, hipStream_t st, const uint8_t *d_q, i32 qlen, i64 n_chunks, u64 n_heavy, bool dense_all, bool sweep_all, size_t ccap, u64 &hits, u64 &maxcand, u64 &occ_all)
{
	const int seed_mode = c->opt.seed_mode;
	u64 *cnt = c->d_cnt.as<u64>();
	const size_t nd = (size_t)n_heavy * GSA_CHUNK;
	if (!dev_ensure<u32>(c, c->dn_lf, nd) || !dev_ensure<u64>(c, c->dn_x0, nd)) return GSA_ERR_NOMEM;
	const u32 *list = dense_all ? (const u32 *)nullptr : c->d_heavy.as<u32>();
#define GSA_DENSE_ARGS(SPAN) dim3((unsigned)(n_heavy * DENSE_WGS(SPAN))), dim3(DENSE_TPB), 0, st, c->di, d_q, qlen, c->prm, list, c->dn_lf.as<u32>(), c->dn_x0.as<u64>(), cnt
#ifdef GSA_EXPERIMENTS
	static const u64 sweep_min = [] { const char *e = getenv("GSA_SWEEP_MIN"); return e ? (u64)atoll(e) : 1024ull; }();
#else
	const u64 sweep_min = 1024;
#endif
	const bool use_sweep = seed_mode != 2 && ((seed_mode == 0 && dense_all) || n_heavy >= sweep_min);      // (-sen: every chunk is dense -- a bundle's worth of them is swept, a short contig's few are searched start by start: one round trip chain of ~5 per start beats a segment's chain of 60-250 when the chip is empty)
	if (sweep_all && seed_mode == 1 && ++c->seed_sweep_run >= c->seed_sweep_period) { c->seed_sweep_next = false; c->seed_sweep_probe = true; c->seed_sweep_run = 0; }      // look again now and then
	if (use_sweep) {
#ifdef GSA_EXPERIMENTS
		static const int seg_env = [] { const char *e = getenv("GSA_SWEEP_SEG"); return e ? atoi(e) : 0; }();
#else
		const int seg_env = 0;
#endif
		const int shape_env = c->opt.sweep_shape;
		// few dense chunks (a bundle of short contigs): one chunk per workgroup of four waves and 40 starts per segment, so that the
		// chip has waves to run; many: four chunks per workgroup of two waves, 160 starts per segment
		const bool small = shape_env >= 0 ? shape_env == 1 : n_heavy < 4096;      // (a 60 Mb -sen bundle, 6 000 chunks: 3.9 ms with four chunks per workgroup, 4.8 with one)
		const int seg = seg_env > 0 ? seg_env : (small ? 40 : 160);
#define GSA_SWEEP_ARGS(NCH_, TPB_) dim3((unsigned)((n_heavy + (NCH_) - 1) / (NCH_))), dim3(TPB_), 0, st, c->di, d_q, qlen, c->prm, list, (u32)n_heavy, c->dn_lf.as<u32>(), c->dn_x0.as<u64>(), cnt, seg
		if (small) { if (c->di.kmer_e16) hipLaunchKernelGGL((k_dense_sweep<true, 1, 256>), GSA_SWEEP_ARGS(1, 256)); else hipLaunchKernelGGL((k_dense_sweep<false, 1, 256>), GSA_SWEEP_ARGS(1, 256)); }
		else { if (c->di.kmer_e16) hipLaunchKernelGGL((k_dense_sweep<true, SWEEP_NCH, SWEEP_TPB>), GSA_SWEEP_ARGS(SWEEP_NCH, SWEEP_TPB)); else hipLaunchKernelGGL((k_dense_sweep<false, SWEEP_NCH, SWEEP_TPB>), GSA_SWEEP_ARGS(SWEEP_NCH, SWEEP_TPB)); }
#undef GSA_SWEEP_ARGS
	}
	else if (dense_all) { if (c->di.kmer_e16) hipLaunchKernelGGL((k_dense_search<true, 512>), GSA_DENSE_ARGS(512)); else hipLaunchKernelGGL((k_dense_search<false, 512>), GSA_DENSE_ARGS(512)); }
	else { if (c->di.kmer_e16) hipLaunchKernelGGL((k_dense_search<true, 256>), GSA_DENSE_ARGS(256)); else hipLaunchKernelGGL((k_dense_search<false, 256>), GSA_DENSE_ARGS(256)); }
#undef GSA_DENSE_ARGS
	hipLaunchKernelGGL(k_dense_resolve, dim3((unsigned)n_heavy), dim3(256), 0, st, list, (u32)n_chunks, qlen, (int)c->prm.bSensitive, c->dn_lf.as<u32>(), c->dn_x0.as<u64>(), cnt,
	                   c->d_cand_s.as<i32>(), c->d_cand_len.as<i32>(), c->d_cand_x0.as<u64>(), c->d_cand_freq.as<i32>(), (u32)ccap, c->d_cand_cnt.as<u32>(), c->d_onpath.as<u32>(),
	                   c->d_chunk_hits.as<i32>(), c->h_cnt, c->d_chunk_base.as<i32>());
	GSA_CHECK(c, hipGetLastError());      // (of the search / sweep launch as well: an error stays until it is read)
	if (c->profiling || c->prof_seed) hipEventRecord(c->ev[1], st);
	GSA_CHECK(c, hipEventRecord(c->ev[21], st));      // (the exclusive prefix of the per-chunk hit counts is left by the kernel's last workgroup)
	GSA_CHECK(c, hipEventSynchronize(c->ev[21]));
	hits += c->h_cnt[CNT_HITS]; if (c->h_cnt[CNT_CAND] > maxcand) maxcand = c->h_cnt[CNT_CAND]; occ_all += c->h_cnt[CNT_OCCBLK_ALL];
	if (dense_all) { c->dbg[0] = 0; c->dbg[1] = n_heavy; c->dbg[2] = c->dbg[3] = c->dbg[4] = c->dbg[5] = 0; c->counters[0] = 0; }
	return GSA_OK;
}
