// gsalign_amd/csrc/k_seed_select.hip -- stage 1 behind the search: the on-chain candidates' hits located (a3) and keyed, the bitmap of
// occupied PosDiff values, ordering by (PosDiff, qPos) and SeedGrouping (a6).
//
// Replaces bwt_sa + SeedGrouping (reference src/GSAlign.cpp:95-107,126-143; src/bwt_search.cpp:129-139).
#include "gsa_ctx.h"
#include "gsa_fm.h"
#include "gsa_scan.h"
#include "gsa_seed.h"

// ---------------------------------------------------------------------------
// Candidate -> seeds: keep the matches whose start lies on the true chain, locate
// every hit through the dense SA (a3: one read instead of ~31 dependent LF steps)
// and emit the 64-bit sort key ((PosDiff + qlen) << qbits) | qPos with the length.
// ---------------------------------------------------------------------------
// One workgroup per chunk.  Phase A: the on-chain candidates get their output ranges by a scan over the candidate index
// (deterministic order).  Phase B: one lane per HIT -- a seed with 100 hits is 100 lanes, not a 100-iteration loop of one
// lane -- which finds its candidate by binary search over the offsets (LDS), locates its row and ranks itself among the
// hits of its start by position: the tie-break of the (group, qPos) order, which the reference gets from a stable sort
// of the PosDiff order (the f rows of one start are re-read by f lanes: L1/L2 hits on the dense SA).
#define SEL_HASH 256
#ifndef SEL_TRIES
#define SEL_TRIES 4      // probes of the workgroup's LDS table of occupied PosDiff words before a hit goes to its word in HBM
#endif
// the coarse bitmap beside the PosDiff bitmap: bit (w >> 5) for bitmap word w (k_chain.hip, OpPdScan)
__device__ __forceinline__ void pd_coarse_set(u32 *pdcb, unsigned long long w)
{
	const unsigned long long blk = w >> 5; const u32 bit = 1u << (blk & 31);
	// (looked at first: the main diagonal of a whole contig sits in one block, and an unconditional atomic per workgroup queues on that word
	//  -- locate + order of a 250 Mb contig 0.31 -> 0.67 ms when tried; a kernel of its own with a thread per hit: 1.4 ms, the looks queue too)
	if (!(__hip_atomic_load(&pdcb[blk >> 5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) atomicOr(&pdcb[blk >> 5], bit);
}
__global__ void __launch_bounds__(256) k_seed_select(DevIndex di, u32 cand_cap, const u32 *__restrict__ cand_cnt, const i32 *__restrict__ cand_s, const i32 *__restrict__ cand_len,
                                                      const u64 *__restrict__ cand_x0, const i32 *__restrict__ cand_freq, const u32 *__restrict__ onpath,
                                                      const i32 *__restrict__ hit_base, Bundle bnd, i32 s_off, int qbits, u64 *key, u32 *val, u32 *pdbm, u32 *pdcb, u32 lds_cand, uint8_t *pdby)
{
	// (bnd.lmax = length of the whole contig, s_off = contig position of the first chunk searched: not 0 when only a chunk range
	//  of the contig was seeded on this GPU, gsa_seed_chunks.  A bundle of contigs: the key's PosDiff is the true one of the
	//  chunk's contig plus that contig's stride, see Bundle)
	// Round 4: the hits leave this kernel in (qPos, rank) order -- chunk after chunk (the launch order), inside a chunk by the start position
	// of their candidate (the on-chain starts are marked in a bitmap over the chunk's positions: a candidate's place is the number of marked
	// starts below its own), inside a start by the rank of the hit.  Stage 2 then needs ONE stable sort by the group id alone (three 8-bit passes
	// instead of eight over the whole 57-bit key).  Off-chain candidates take no part.
	extern __shared__ u32 s_offs[];                    // [nc + 1] exclusive prefix of the hit counts of the on-chain candidates in start order | [nc] their candidate numbers
	u32 *s_ord = s_offs + lds_cand + 2;                // (lds_cand: the most candidates any chunk of THIS contig holds -- not the capacity of the segments)
	__shared__ unsigned long long s_w[SEL_HASH]; __shared__ u32 s_b[SEL_HASH];
	__shared__ u32 s_wsum[4], s_run, s_sb[GSA_CHUNK / 32 + 2], s_sbpre[GSA_CHUNK / 32 + 2];
	const u32 chunk = blockIdx.x, nc = cand_cnt[chunk];
	const size_t cbase = (size_t)chunk * cand_cap;
	const int j = threadIdx.x, lane = j & 63, wv = j >> 6;
	for (int t = j; t < SEL_HASH; t += 256) { s_w[t] = ~0ull; s_b[t] = 0; }
	for (int t = j; t < GSA_CHUNK / 32 + 2; t += 256) s_sb[t] = 0;
	if (j == 0) s_run = 0;
	__syncthreads();
	for (u32 i = j; i < nc; i += 256) {
		const i32 p = cand_s[cbase + i] - (i32)chunk * GSA_CHUNK;
		if ((onpath[(size_t)chunk * PATH_WORDS + (p >> 5)] >> (p & 31)) & 1u) atomicOr(&s_sb[p >> 5], 1u << (p & 31));
	}
	__syncthreads();
	if (wv == 0) {      // marked starts below each word: 313 words, five per lane
		constexpr int WPL = (GSA_CHUNK / 32 + 2 + 63) / 64;
		u32 c5 = 0;
		for (int k = 0; k < WPL; k++) { const int w = lane * WPL + k; if (w < GSA_CHUNK / 32 + 2) c5 += (u32)__popc(s_sb[w]); }
		u32 inc = c5;
		for (int o = 1; o < 64; o <<= 1) { const u32 t = __shfl_up(inc, o); if (lane >= o) inc += t; }
		u32 run = inc - c5;
		for (int k = 0; k < WPL; k++) { const int w = lane * WPL + k; if (w < GSA_CHUNK / 32 + 2) { s_sbpre[w] = run; run += (u32)__popc(s_sb[w]); } }
		if (lane == 63) s_run = inc;      // on-chain candidates of the chunk
	}
	__syncthreads();
	const u32 n_on = s_run;
	for (u32 i = j; i < nc; i += 256) {
		const i32 p = cand_s[cbase + i] - (i32)chunk * GSA_CHUNK;
		if ((s_sb[p >> 5] >> (p & 31)) & 1u) {
			if ((onpath[(size_t)chunk * PATH_WORDS + (p >> 5)] >> (p & 31)) & 1u) {
				const u32 o = s_sbpre[p >> 5] + (u32)__popc(s_sb[p >> 5] & ((1u << (p & 31)) - 1u));
				s_ord[o] = i;
			}
		}
	}
	__syncthreads();
	if (j == 0) s_run = 0;
	__syncthreads();
	for (u32 i0 = 0; i0 < n_on; i0 += 256) {
		const u32 o = i0 + j;
		const u32 f = o < n_on ? (u32)cand_freq[cbase + s_ord[o]] : 0u;
		u32 inc = f;
		for (int oo = 1; oo < 64; oo <<= 1) { const u32 t = __shfl_up(inc, oo); if (lane >= oo) inc += t; }
		if (lane == 63) s_wsum[wv] = inc;
		__syncthreads();
		u32 wo = 0; for (int w = 0; w < wv; w++) wo += s_wsum[w];
		const u32 run = s_run;
		if (o < n_on) s_offs[o] = run + wo + inc - f;
		__syncthreads();
		if (j == 255) s_run = run + wo + inc;
		__syncthreads();
	}
	const u32 total = s_run;
	if (j == 0) s_offs[n_on] = total;
	__syncthreads();
	const u64 base = (u64)hit_base[chunk];
	i64 pd_base = bnd.lmax;                              // key = rPos - qPos + pd_base
	if (bnd.n) { const i32 ci = bnd.chunk_contig[chunk]; pd_base += (i64)bnd.off[ci] + (i64)ci * bnd.pds; }
	__shared__ unsigned long long s_r[256];                  // located positions of the 256 hits in flight: a hit ranks itself among its siblings from here
	for (u32 t0 = 0; t0 < total; t0 += 256) {
		const u32 t = t0 + j;
		u32 i = 0, h = 0, f = 0, len = 0; i32 s = 0; u64 x0 = 0, r = 0;
		if (t < total) {
			// the candidate whose range holds hit t: the last i with s_offs[i] <= t (empty ranges share their start with the next one)
			u32 lo = 0, hi = n_on;
			while (hi - lo > 1) { const u32 mid = (lo + hi) >> 1; if (s_offs[mid] <= t) lo = mid; else hi = mid; }
			i = s_ord[lo]; h = t - s_offs[lo];
			s = cand_s[cbase + i] + s_off; f = (u32)cand_freq[cbase + i]; len = (u32)cand_len[cbase + i]; x0 = cand_x0[cbase + i];
			r = (x0 >> 63) ? (x0 & ~(1ull << 63)) : fm_locate(di, x0 + h);      // (bit 63: a unique match whose text position the sweep already knows)
		}
		s_r[j] = r;
		__syncthreads();
		if (t < total) {
			const i64 pd = (i64)r - s + pd_base;
			u32 rank = 0;
			if (f > 1) {
				const u32 first = t - h;                            // hit index of sibling 0
				for (u32 h2 = 0; h2 < f; h2++) {
					const u32 ts = first + h2;
					const u64 r2 = (ts >= t0 && ts < t0 + 256) ? s_r[ts - t0] : fm_locate(di, x0 + h2);      // (siblings in another window of 256: the dense SA again)
					rank += r2 < r ? 1u : 0u;
				}
			}
			const u64 at = base + (t - h) + rank;                 // (the hits of a start in rank order: distinct text positions, so the ranks are a permutation)
			key[at] = ((u64)pd << qbits) | (u32)s;
			val[at] = len | (rank << 16);
			// occupied PosDiff values: groups without sorting by PosDiff (k_chain.hip).  Collected per workgroup in LDS, one
			// global OR per touched word at the end: a chunk's hits sit in two or three words and the whole contig's main
			// diagonal in one cache line -- an atomic (or even a look) per hit queues 75 k operations on that line.  Hits of
			// repeats scatter over the genome: after a few probes they go straight to their own (uncontended) word.
			// (round 5) where the hits scatter -- -sen: a chunk holds thousands of chance hits on as many words, and a device-scope atomic each is what `locate` then
			// costs (9.7 M of them in a 60 Mb bundle, 2.8 ms) -- a byte per PosDiff value takes a plain store; k_pd_pack makes the bitmap of it
			if (pdby) pdby[pd] = 1;
			else if (pdbm) {
				const unsigned long long w = (unsigned long long)(pd >> 5); const u32 bit = 1u << (pd & 31);
				int hh = (int)((w * 0x9E3779B1ull) >> 7) & (SEL_HASH - 1), tries = 0;
				for (; tries < SEL_TRIES; tries++, hh = (hh + 1) & (SEL_HASH - 1)) {
					const unsigned long long prev = atomicCAS(&s_w[hh], ~0ull, w);
					if (prev == ~0ull || prev == w) { atomicOr(&s_b[hh], bit); break; }
				}
				if (tries == SEL_TRIES) { atomicOr(&pdbm[w], bit); pd_coarse_set(pdcb, w); }
			}
		}
		__syncthreads();
	}
	if (pdbm && !pdby) {
		__syncthreads();
		for (int t = j; t < SEL_HASH; t += 256) if (s_w[t] != ~0ull) { atomicOr(&pdbm[s_w[t]], s_b[t]); pd_coarse_set(pdcb, s_w[t]); }
	}
}

// The byte map of occupied PosDiff values -> the bitmap and its coarse bitmap, and the bytes back to zero.  A workgroup per 1 024 bitmap words (32 KB of
// bytes, one coarse word): a thread reads the 32 bytes of a word, gathers their low bits (the bytes are 0 or 1: one multiplication per four), stores the
// word if it holds a hit and clears its bytes; the coarse bits are the waves' ballots.  The bitmap is all zero when the pass starts (the invariant of
// stage 2: k_pd_gather clears what a contig set), so plain stores do.
__device__ __forceinline__ u32 pd_nib(u32 x) { return ((x * 0x01020408u) >> 24) & 15u; }      // bytes b0..b3 in {0, 1} -> b0 | b1 << 1 | b2 << 2 | b3 << 3 (no two partial products share a bit)
__global__ void __launch_bounds__(256) k_pd_pack(uint8_t *pdby, i64 nw, u32 *pdbm, u32 *pdcb)
{
	__shared__ u32 s_c[4];
	const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
	const i64 n_tiles = (nw + 1023) >> 10;
	for (i64 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
		u32 cb = 0;
		uint4 a[4], b[4];
#pragma unroll
		for (int k = 0; k < 4; k++) {
			const i64 w = (tile << 10) + k * 256 + tid;
			a[k] = make_uint4(0, 0, 0, 0); b[k] = a[k];
			if (w < nw) { a[k] = ((const uint4 *)pdby)[2 * w]; b[k] = ((const uint4 *)pdby)[2 * w + 1]; }
		}
#pragma unroll
		for (int k = 0; k < 4; k++) {
			const i64 w = (tile << 10) + k * 256 + tid;
			const bool any = (a[k].x | a[k].y | a[k].z | a[k].w | b[k].x | b[k].y | b[k].z | b[k].w) != 0;
			if (any) {
				const u32 word = pd_nib(a[k].x) | (pd_nib(a[k].y) << 4) | (pd_nib(a[k].z) << 8) | (pd_nib(a[k].w) << 12) | (pd_nib(b[k].x) << 16) | (pd_nib(b[k].y) << 20) | (pd_nib(b[k].z) << 24) | (pd_nib(b[k].w) << 28);
				pdbm[w] = word;
				((uint4 *)pdby)[2 * w] = make_uint4(0, 0, 0, 0); ((uint4 *)pdby)[2 * w + 1] = make_uint4(0, 0, 0, 0);
			}
			const unsigned long long m = __ballot(any);      // 64 words = two blocks of 32
			cb |= ((m & 0xffffffffull) ? 1u : 0u) << (k * 8 + wv * 2);
			cb |= ((m >> 32) ? 1u : 0u) << (k * 8 + wv * 2 + 1);
		}
		if (lane == 0) s_c[wv] = cb;
		__syncthreads();
		if (tid == 0) { const u32 v = s_c[0] | s_c[1] | s_c[2] | s_c[3]; if (v) pdcb[tile] = v; }
		__syncthreads();
	}
}

// PosDiff bitmap bits of hits that arrived from another GPU (gsa_import_hits)
__global__ void __launch_bounds__(256) k_pd_from_keys(i64 n, const u64 *__restrict__ key, int qbits, u32 *pdbm, u32 *pdcb)
{
	const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const u64 pd = key[i] >> qbits;
	atomicOr(&pdbm[pd >> 5], 1u << (pd & 31)); pd_coarse_set(pdcb, (unsigned long long)(pd >> 5));
}

// Accounting build only: the LF steps bwt_sa would walk for every located hit (the row is sampled every 32 ROWS, so the
// walk ends at the first row divisible by 32: bwt_search.cpp:129-139).  The hot path reads the dense SA instead; this
// is the algorithmic figure of SURVEY.md section 8(d).
__global__ void __launch_bounds__(256) k_count_lf(DevIndex di, u32 cand_cap, const u32 *__restrict__ cand_cnt, const i32 *__restrict__ cand_s, const u64 *__restrict__ cand_x0,
                                                   const i32 *__restrict__ cand_freq, const u32 *__restrict__ onpath, unsigned long long *out)
{
	const u32 chunk = blockIdx.x, nc = cand_cnt[chunk];
	const size_t cbase = (size_t)chunk * cand_cap;
	unsigned long long steps = 0;
	for (u32 i = threadIdx.x; i < nc; i += blockDim.x) {
		const i32 p = cand_s[cbase + i] - (i32)chunk * GSA_CHUNK;
		if (!((onpath[(size_t)chunk * PATH_WORDS + (p >> 5)] >> (p & 31)) & 1u)) continue;
		const u32 f = (u32)cand_freq[cbase + i];
		for (u32 h = 0; h < f; h++) { u32 st = 0; (void)fm_locate_walk(di, cand_x0[cbase + i] + h, st); steps += st; }
	}
	for (int o = 32; o; o >>= 1) steps += __shfl_down(steps, o);
	if ((threadIdx.x & 63) == 0 && steps) atomicAdd(out, steps);
}

// sorted keys -> SoA seeds + group ids (SeedGrouping, a6): one fused pass (gsa_scan.h); a new group
// starts where PosDiff jumps by more than MaxIndelSize
struct OpDecodeGroup {
	i64 n; const u64 *key; const u32 *val; Bundle bnd; int qbits; i32 max_indel;
	i32 *s_q, *s_len; i64 *s_r; i32 *s_gid, *g_beg, *mail;
	__device__ i32 value(i64 i, int) const
	{
		if (i == 0) return 1;
		const i64 pd = (i64)(key[i] >> qbits), pd0 = (i64)(key[i - 1] >> qbits);      // (a bundle: the stride between contigs exceeds max_indel)
		return (pd - pd0 > max_indel) ? 1 : 0;
	}
	__device__ void emit(i64 i, const i32 *v, const i32 *ex) const
	{
		const u64 k = key[i];
		const i32 qp = (i32)(k & ((1ull << qbits) - 1)); i64 pd = (i64)(k >> qbits) - bnd.lmax;
		if (bnd.n) { const i32 ci = bnd.chunk_contig[qp / GSA_CHUNK]; pd -= (i64)bnd.off[ci] + (i64)ci * bnd.pds; }      // rPos - qp
		s_q[i] = qp; s_len[i] = (i32)(val[i] & 0xffffu); s_r[i] = pd + qp;
		const i32 g = ex[0] + v[0] - 1;
		s_gid[i] = g;
		if (v[0]) g_beg[g] = (i32)i;
	}
	__device__ void done(const i32 *t) const { g_beg[t[0]] = (i32)n; mail[M_NG] = t[0]; }
};

// grow a device buffer keeping its first `keep` elements
template <class T> static T *dev_grow_keep(gsa_ctx *c, DevBuf &b, size_t n, size_t keep)
{
	if ((n ? n : 1) * sizeof(T) <= b.cap) return (T *)b.p;
	DevBuf nb;
	if (!dev_ensure<T>(c, nb, n + n / 2)) return nullptr;
	if (keep && b.p) { if (hipMemcpyAsync(nb.p, b.p, keep * sizeof(T), hipMemcpyDeviceToDevice, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) { hipFree(nb.p); gsa_fail(c, GSA_ERR_HIP, "hipMemcpyAsync"); return nullptr; } }
	if (b.p) { ctx_quiesce(c); hipFree(b.p); }
	b = nb;
	return (T *)b.p;
}

// Groups without the PosDiff sort: decide whether the bitmap of occupied PosDiff values is kept for this contig and clear it
int prepare_pd_bitmap(gsa_ctx *c, i64 n_hits, i64 n_chunks)
{
	const u64 pd_words = ((u64)c->pd_span >> 5) + 2;
	// (a chunk range: the hit count of the whole contig is not known here; the bitmap is kept whenever MaxIndelSize allows it)
	// (since the scan only visits occupied blocks -- OpPdScan, round 4 -- the bitmap pays whatever the hit count: a human reference is 776 MB per
	//  contig; beyond 2 GB -- bundles against a large reference -- only with enough hits to justify the memory)
	c->pd_path = (n_hits > 0 || c->split) && c->prm.MaxIndelSize >= 0 && c->prm.MaxIndelSize <= 31 && (c->split || pd_words <= (512ull << 20) || pd_words <= 64ull * (u64)n_hits + 65536) && c->opt.pd_bitmap;
	c->seed_view_ready = false;
	if (c->pd_path) {
		const size_t cap0 = c->d_pdbm.cap;
		const size_t ccap0 = c->d_pdcb.cap;
		if (!dev_ensure<u32>(c, c->d_pdbm, (size_t)pd_words + 66) || !dev_ensure<u32>(c, c->d_pdcb, (size_t)(pd_words >> 10) + 4)) {
			// no room for the bitmap (up to 2 GB per context): this contig's groups come from the PosDiff sort instead (seed_view_sort), as
			// for MaxIndelSize > 31 -- slower, same result
			(void)hipGetLastError(); c->err.clear(); c->pd_path = false; c->pdbm_dirty = true;
			return GSA_OK;
		}
		if (c->d_pdbm.cap != cap0 || c->pdbm_dirty) GSA_CHECK(c, hipMemsetAsync(c->d_pdbm.p, 0, c->d_pdbm.cap, c->stream));
		if (c->d_pdcb.cap != ccap0 || c->pdbm_dirty) GSA_CHECK(c, hipMemsetAsync(c->d_pdcb.p, 0, c->d_pdcb.cap, c->stream));
		c->pdbm_dirty = true; c->pd_words = (i64)pd_words;
		// the byte map (Options::pd_bytes): where a chunk's hits overflow the workgroup's table of words (256) and the pass over the bytes costs less than their atomics would
		c->pd_bytes = false;
		if (!c->split && n_chunks > 0 && (c->opt.pd_bytes == 2 || (c->opt.pd_bytes == 1 && n_hits >= 512 * n_chunks && pd_words * 32 <= 256ull * (u64)n_hits && pd_words <= (128ull << 20)))) {      // (at most 4 GB of bytes per context)
			const size_t bcap0 = c->d_pdby.cap;
			if (dev_ensure<uint8_t>(c, c->d_pdby, ((size_t)pd_words + 66) * 32)) {
				if (c->d_pdby.cap != bcap0) GSA_CHECK(c, hipMemsetAsync(c->d_pdby.p, 0, c->d_pdby.cap, c->stream));
				c->pd_bytes = true;
			} else { (void)hipGetLastError(); c->err.clear(); }      // (no room: the atomics do it)
		}
	}
	return GSA_OK;
}

// The tail of stage1_seed once the search kernels are through (the host has waited for them): the hits of the on-chain candidates, located and keyed,
// the PosDiff bitmap, and -- unless the contig is split over GPUs -- the groups.
int stage1_select(gsa_ctx *c, i64 n_chunks, i64 n_hits, size_t ccap, u64 contig_maxcand, i32 s_off, u64 occ_all)
{
	hipStream_t st = c->stream;
	const bool split = c->split;
	const size_t hcap = (size_t)n_hits + 64;
	// Groups: a new group starts where the sorted PosDiff values jump by more than MaxIndelSize.  With a bitmap of the
	// occupied PosDiff values that needs no sort: group id = number of group starts at or below a hit's PosDiff (a scan
	// over the bitmap, stage 2).  The PosDiff-sorted view of the seeds (stage-1 view of the C ABI) is then built on demand.
	if (int rcp = prepare_pd_bitmap(c, n_hits, n_chunks)) return rcp;
	if (n_hits > 0) {
		if (!dev_ensure<u64>(c, c->d_key_a, hcap) || !dev_ensure<u32>(c, c->d_val_a, hcap)) return GSA_ERR_NOMEM;
		// (LDS by the contig's own maximum: the segments' capacity only grows -- one contig with a crowded chunk, or the counting pass of the
		//  bench, and every later launch would run one workgroup per CU)
		const size_t sel_cand = contig_maxcand < ccap ? (((size_t)contig_maxcand + 64) & ~(size_t)63) : ccap;
		hipLaunchKernelGGL(k_seed_select, dim3((unsigned)n_chunks), dim3(256), 2 * (sel_cand + 2) * sizeof(u32), st, c->di, (u32)ccap, c->d_cand_cnt.as<u32>(), c->d_cand_s.as<i32>(), c->d_cand_len.as<i32>(),
		                   c->d_cand_x0.as<u64>(), c->d_cand_freq.as<i32>(), c->d_onpath.as<u32>(), c->d_chunk_base.as<i32>(), c->bnd, s_off, c->qbits, c->d_key_a.as<u64>(), c->d_val_a.as<u32>(), c->pd_path ? c->d_pdbm.as<u32>() : (u32 *)nullptr, c->d_pdcb.as<u32>(), (u32)sel_cand, (c->pd_path && c->pd_bytes) ? c->d_pdby.as<uint8_t>() : (uint8_t *)nullptr);
		if (c->pd_path && c->pd_bytes) {
			const i64 tiles = (c->pd_words + 1023) >> 10;
			hipLaunchKernelGGL(k_pd_pack, dim3((unsigned)(tiles < 4096 ? tiles : 4096)), dim3(256), 0, st, c->d_pdby.as<uint8_t>(), c->pd_words, c->d_pdbm.as<u32>(), c->d_pdcb.as<u32>());
		}
	}
	if (c->profiling) hipEventRecord(c->ev[2], st);
	u64 lf_steps = 0;
	if (c->count_blocks && n_hits > 0) {
		unsigned long long *d_lf = (unsigned long long *)(c->d_mail.as<i32>() + M_LFSTEPS);
		GSA_CHECK(c, hipMemsetAsync(d_lf, 0, 8, st));
		hipLaunchKernelGGL(k_count_lf, dim3((unsigned)n_chunks), dim3(256), 0, st, c->di, (u32)ccap, c->d_cand_cnt.as<u32>(), c->d_cand_s.as<i32>(), c->d_cand_x0.as<u64>(),
		                   c->d_cand_freq.as<i32>(), c->d_onpath.as<u32>(), d_lf);
		GSA_CHECK(c, hipMemcpyAsync(&c->h_cnt[CNT_DONE], d_lf, 8, hipMemcpyDeviceToHost, st));      // (h_cnt[CNT_DONE] is always 0 after the seed kernel: a free pinned slot)
		GSA_CHECK(c, hipStreamSynchronize(st));
		lf_steps = c->h_cnt[CNT_DONE];
	}
	c->counters[1] = lf_steps; c->counters[2] = (u64)n_hits; c->counters[3] = (u64)n_hits; c->counters[7] = occ_all;
	c->n_seeds = n_hits; c->hits_sorted = !split;
	if (split) return GSA_OK;                 // (the tail of stage 1 runs in gsa_finish_contig, on the hits of all ranges)
	if (n_hits == 0) { if (c->profiling) { GSA_CHECK(c, hipStreamSynchronize(st)); float ms; hipEventElapsedTime(&ms, c->ev[0], c->ev[1]); c->kernel_ms[0] = ms; } return GSA_OK; }
	if (n_hits >= (1ll << 31) - 2) return gsa_fail(c, GSA_ERR_LIMIT, "more than 2^31 seeds in one contig");
	if (c->pd_path) {
		if (c->profiling) hipEventRecord(c->ev[3], st);
		c->n_groups = -1; c->ev_pending |= 1;
		return GSA_OK;
	}
	return seed_view_sort(c);
}

// Seeds in PosDiff order with their group ids (CompByPosDiff + SeedGrouping, a5/a6): always for the stage-1 view of
// the C ABI, and as the front of stage 2 when the PosDiff bitmap does not apply.
int seed_view_sort(gsa_ctx *c)
{
	if (c->seed_view_ready || c->n_seeds == 0) return GSA_OK;
	hipStream_t st = c->stream;
	const size_t n = (size_t)c->n_seeds, hcap = n + 64;
	if (!dev_ensure<u64>(c, c->d_key_b, hcap) || !dev_ensure<u32>(c, c->d_val_b, hcap)) return GSA_ERR_NOMEM;
	int rc = gsa_sort_pairs_u64_u32(c, c->d_key_a.as<u64>(), c->d_key_b.as<u64>(), c->d_val_a.as<u32>(), c->d_val_b.as<u32>(), n, 0, c->qbits + c->pdbits);
	if (rc) return rc;
	if (!dev_ensure<i32>(c, c->s_q, n) || !dev_ensure<i32>(c, c->s_len, n) || !dev_ensure<i64>(c, c->s_r, n) || !dev_ensure<i32>(c, c->s_gid, n) ||
	    !dev_ensure<i32>(c, c->d_flag, n + 1) || !dev_ensure<i32>(c, c->d_scan, n + 1) || !dev_ensure<i32>(c, c->g_beg, n + 1)) return GSA_ERR_NOMEM;
	{
		OpDecodeGroup op = { (i64)n, c->d_key_b.as<u64>(), c->d_val_b.as<u32>(), c->bnd, c->qbits, c->prm.MaxIndelSize,
		                     c->s_q.as<i32>(), c->s_len.as<i32>(), c->s_r.as<i64>(), c->s_gid.as<i32>(), c->g_beg.as<i32>(), c->d_mail.as<i32>() };
		rc = lb_launch<1>(c, (i64)n, op);
		if (rc) return rc;
	}
	if (c->profiling && !c->pd_path) hipEventRecord(c->ev[3], st);
	// the group count stays on the device (mailbox); nothing downstream needs it on the host
	c->n_groups = -1;
	if (!c->pd_path) c->ev_pending |= 1;
	c->seed_view_ready = true;
	return GSA_OK;
}

// hits of another GPU's chunk range behind this context's own ones (keys / vals: host or device memory)
int stage1_import_hits(gsa_ctx *c, const u64 *keys, const u32 *vals, i64 n)
{
	if (n <= 0) return GSA_OK;
	if (c->n_seeds + n >= (1ll << 31) - 2) return gsa_fail(c, GSA_ERR_LIMIT, "more than 2^31 seeds in one contig");
	const size_t have = (size_t)c->n_seeds, want = have + (size_t)n + 64;
	if (!dev_grow_keep<u64>(c, c->d_key_a, want, have) || !dev_grow_keep<u32>(c, c->d_val_a, want, have)) return GSA_ERR_NOMEM;
	// (host memory, memory of this GPU, or of another GPU of the node -- then the copy goes peer to peer over xGMI)
	int src_dev = -1;
	{ hipPointerAttribute_t at; if (hipPointerGetAttributes(&at, keys) == hipSuccess && at.type == hipMemoryTypeDevice) src_dev = at.device; else (void)hipGetLastError(); }
	if (src_dev >= 0 && src_dev != c->device) {
		int can = 0; (void)hipDeviceCanAccessPeer(&can, c->device, src_dev);
		if (can) { hipError_t e = hipDeviceEnablePeerAccess(src_dev, 0); if (e != hipSuccess) (void)hipGetLastError(); }      // (already enabled is fine)
		GSA_CHECK(c, hipMemcpyPeerAsync(c->d_key_a.as<u64>() + have, c->device, keys, src_dev, (size_t)n * 8, c->stream));
		GSA_CHECK(c, hipMemcpyPeerAsync(c->d_val_a.as<u32>() + have, c->device, vals, src_dev, (size_t)n * 4, c->stream));
	} else {
		GSA_CHECK(c, hipMemcpyAsync(c->d_key_a.as<u64>() + have, keys, (size_t)n * 8, hipMemcpyDefault, c->stream));
		GSA_CHECK(c, hipMemcpyAsync(c->d_val_a.as<u32>() + have, vals, (size_t)n * 4, hipMemcpyDefault, c->stream));
	}
	if (c->pd_path) hipLaunchKernelGGL(k_pd_from_keys, dim3(grid_for((size_t)n, 256)), dim3(256), 0, c->stream, n, c->d_key_a.as<u64>() + have, c->qbits, c->d_pdbm.as<u32>(), c->d_pdcb.as<u32>());
	GSA_CHECK(c, hipGetLastError());
	GSA_CHECK(c, hipStreamSynchronize(c->stream));      // (the caller's buffers are free again)
	c->n_seeds += n;
	return GSA_OK;
}

// the tail of stage 1 once the hits of every chunk range are here
int stage1_finish_split(gsa_ctx *c)
{
	c->counters[2] = c->counters[3] = (u64)c->n_seeds;
	c->seed_view_ready = false;
	if (c->n_seeds == 0) return GSA_OK;
	if (c->pd_path) { c->n_groups = -1; return GSA_OK; }
	return seed_view_sort(c);
}

// Stage 2 consumed the PosDiff bitmap (k_pd_gather clears the words it read); a second stage 2 on the same hits needs it back.
int stage1_restore_pdbm(gsa_ctx *c)
{
	if (!c->pd_path || c->n_seeds == 0) return GSA_OK;
	if (c->pdbm_dirty) { GSA_CHECK(c, hipMemsetAsync(c->d_pdbm.p, 0, c->d_pdbm.cap, c->stream)); GSA_CHECK(c, hipMemsetAsync(c->d_pdcb.p, 0, c->d_pdcb.cap, c->stream)); }
	hipLaunchKernelGGL(k_pd_from_keys, dim3(grid_for((size_t)c->n_seeds, 256)), dim3(256), 0, c->stream, c->n_seeds, c->d_key_a.as<u64>(), c->qbits, c->d_pdbm.as<u32>(), c->d_pdcb.as<u32>());
	GSA_CHECK(c, hipGetLastError());
	c->pdbm_dirty = true;
	return GSA_OK;
}
