// gsalign_amd/csrc/gsa_walk.h -- what the passes over a stage-8 result share (k_variants.hip, k_cigar.hip, k_cs.hip, k_lift.hip, k_track.hip, k_segs.hip, k_proj.hip,
// k_regions.hip, k_qtrack.hip): the inputs of a record walk and the op string of a gap record, one step of a gap's columns by a lane and by a wavefront, the "=" / "X"
// rule, the search for the block of a work item, the two levels of the exclusive scan, the span table of the passes that ask where a block lies on the reference (its
// host builder, the cover search, the record of a text position), and on the host the blocks of one contig of the result.  What a pass makes of a record -- which
// records it walks, what a column means -- stays with the pass.
#ifndef GSA_WALK_H
#define GSA_WALK_H
#include <algorithm>
#include <cstring>
#include "gsa_ctx.h"
#include "gsa_fm.h"
#include "gsa_gap.h"

#define WALK_SERIAL 64      // gap records of at most this many columns are walked by one lane, longer ones by a wavefront in 64-column steps

// what every record walk reads
struct GapIn {
	const gsa_frag *frag; const i32 *ftype, *fjob;
	const i32 *j_nops; const i64 *j_opsoff; const uint8_t *j_ops;      // DP jobs of the job list
	const i32 *e_nops; const i64 *e_opsoff; const uint8_t *e_ops;      // DP jobs launched early from the leaf table (fjob <= -2)
	const uint8_t *query, *ref;
};

static inline void gap_in_fill(const gsa_ctx *c, GapIn &a)
{
	a.frag = c->f_rec.as<gsa_frag>(); a.ftype = c->f_type.as<i32>(); a.fjob = c->f_job.as<i32>();
	a.j_nops = c->j_nops.as<i32>(); a.j_opsoff = c->j_opsoff.as<i64>(); a.j_ops = c->d_ops.as<uint8_t>();
	a.e_nops = c->e_nops.as<i32>(); a.e_opsoff = c->e_opsoff.as<i64>(); a.e_ops = c->e_ops.as<uint8_t>();
	a.query = c->q_dev; a.ref = c->di.ref;
}

// The columns of gap record i (type ftype: FT_DP or FT_EQ, both sides non-empty): op[0 .. L) is the forward M/D/I string of its DP job; an equal-length gap
// that needed no DP has none (op stays as the caller set it: null) and is L = qlen columns of 'M'.  false: a DP record without a DP job -- cannot happen
// (OpDpJobs gives every FT_DP record a job >= 0 or an early job <= -2); the passes count and report it, never skip it silently.
__device__ __forceinline__ bool gap_ops(const GapIn &a, i64 i, i32 ftype, const gsa_frag &f, const uint8_t *&op, i32 &L)
{
	if (ftype != FT_DP) { L = f.qlen; return true; }
	const i32 fj = a.fjob[i];
	if (fj >= 0) { op = a.j_ops + a.j_opsoff[fj]; L = a.j_nops[fj]; return true; }
	if (fj <= -2) { const i32 e = -2 - fj; op = a.e_ops + a.e_opsoff[e]; L = a.e_nops[e]; return true; }
	return false;
}

// one column of a walk by ONE lane is behind it: 'D' consumes no reference base, 'I' no query base
__device__ __forceinline__ void col_advance(int ch, i64 &rp, i32 &qp) { if (ch != 'D') rp++; if (ch != 'I') qp++; }

// a column that holds a base in both rows: true 'X', false '=' (an ambiguous base matches nothing, itself included)
__device__ __forceinline__ bool col_mismatch(uint8_t r, uint8_t q) { const int x = gsa_nt4(r); return !(x < 4 && x == gsa_nt4(q)); }

// One step of a gap's columns (op[0 .. L), null: 'M' throughout) by a whole wavefront, 64 columns from `base`: the lane's column p, its op ch (0 past the end), whether it
// consumes a reference / a query base (c1 / c2), and its positions -- the step's (rp0, qp0) plus the number of lower lanes whose column consumes a base of that side.
// rp0 / qp0 leave as the next step's.  No LDS, no barrier; the whole wavefront calls it
struct WaveCol { i32 p; int ch; bool c1, c2; i64 rp; i32 qp; };
__device__ __forceinline__ WaveCol wave_step(const uint8_t *op, i32 L, i32 base, i64 &rp0, i32 &qp0)
{
	const int lane = threadIdx.x & 63;
	const unsigned long long below = (1ull << lane) - 1ull;
	WaveCol w;
	w.p = base + lane;
	w.ch = w.p < L ? (op ? (int)op[w.p] : (int)'M') : 0;
	w.c1 = w.ch == 'M' || w.ch == 'I'; w.c2 = w.ch == 'M' || w.ch == 'D';
	const unsigned long long m1 = __ballot(w.c1), m2 = __ballot(w.c2);
	w.rp = rp0 + __popcll(m1 & below); w.qp = qp0 + __popcll(m2 & below);
	rp0 += __popcll(m1); qp0 += __popcll(m2);
	return w;
}

// one block of the result, ALL of them, in result order: first record (absolute), records, strand, first work item; entry [nb]: wbase = W  (k_cigar.hip's
// block table d_cblk, read by k_cs.hip too)
struct CigBlk { i64 frag_off; i32 n_frag, bdir, wbase, _pad; };

// the last of t[0 .. n) whose key is <= x, 0 when there is none (entries that share a key -- blocks without records, without ops -- : the last of them)
// (B: T, or the base of T that holds the key)
template <class T, class B, class K>
__device__ __forceinline__ i32 blk_last_le(const T *t, i32 n, K B::*key, i64 x)
{
	i32 lo = 0, hi = n;
	while (hi - lo > 1) { const i32 m = (lo + hi) >> 1; if (t[m].*key <= x) lo = m; else hi = m; }
	return lo;
}

// Exclusive scan over a workgroup of 256 threads, N values per thread at once: v[a] -> the sum of v[a] of the threads below.  s_w: 4 N entries, which hold
// the wavefronts' sums afterwards (array a at s_w[4 a ..]).  One barrier; a caller that scans again with the same s_w puts one of its own in between.
template <class T, int N>
__device__ __forceinline__ void wg_excl_scan(T (&v)[N], T *s_w)
{
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
	T s[N];
	for (int a = 0; a < N; a++) s[a] = v[a];
	for (int d = 1; d < 64; d <<= 1)
		for (int a = 0; a < N; a++) { const T x = __shfl_up(s[a], d); if (lane >= d) s[a] += x; }
	if (lane == 63) for (int a = 0; a < N; a++) s_w[4 * a + wv] = s[a];
	__syncthreads();
	for (int a = 0; a < N; a++) { T pre = 0; for (int k = 0; k < wv; k++) pre += s_w[4 * a + k]; v[a] = pre + s[a] - v[a]; }
}
template <class T>
__device__ __forceinline__ T wg_excl_scan(T v, T *s_w) { T a[1] = { v }; wg_excl_scan(a, s_w); return a[0]; }

// second level of a pass's scan, by ONE workgroup of 256: x[0 .. nwg), the workgroups' sums, -> their exclusive prefixes, in tiles of 256 with a carry; returns the total
__device__ __forceinline__ i64 wg_scan_sums(i64 *x, i64 nwg, i64 *s_w)
{
	i64 carry = 0;
	for (i64 base = 0; base < nwg; base += 256) {
		const i64 i = base + threadIdx.x;
		const i64 e = wg_excl_scan<i64>(i < nwg ? x[i] : 0, s_w);
		if (i < nwg) x[i] = carry + e;
		carry += s_w[0] + s_w[1] + s_w[2] + s_w[3];
		__syncthreads();
	}
	return carry;
}

// the workgroup's number of set flags -> wg[blockIdx.x] (s_w: 4 entries; one barrier)
__device__ __forceinline__ void wg_count(bool hit, i32 *s_w, i64 *wg)
{
	i32 tot = hit ? 1 : 0;
	for (int d = 32; d; d >>= 1) tot += __shfl_xor(tot, d);
	if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = tot;
	__syncthreads();
	if (threadIdx.x == 0) wg[blockIdx.x] = (i64)s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// n into field f of v[4] (by selects: a run-time index would put the array into scratch)
__device__ __forceinline__ void win_add(u32 v[4], int f, u32 n)
{
#pragma unroll
	for (int k = 0; k < 4; k++) v[k] += k == f ? n : 0u;
}

// The lanes' counts v[4] for window key (-1: none) into a dense array of four counts per window (k_track.hip, k_qtrack.hip): reduced over runs of equal keys in
// neighbouring lanes first (a run starts where the key differs from the lane below; equal keys further apart simply make two runs), then one atomicAdd per
// (run, field).  The whole wavefront calls it.
__device__ __forceinline__ void win_flush(u32 *bin, i64 nbin, i32 key, u32 v[4])
{
	const int lane = threadIdx.x & 63;
	const i32 pk = __shfl_up(key, 1);
	const bool head = lane == 0 || pk != key;
	const unsigned long long hm = __ballot(head);
	if (__ballot(key >= 0) == 0ull) return;
	const unsigned long long above = lane == 63 ? 0ull : (hm >> (lane + 1));
	const int nh = above ? lane + __ffsll((long long)above) : 64;      // the next run's first lane
	for (int d = 1; d < 64; d <<= 1)
#pragma unroll
		for (int f = 0; f < 4; f++) { const u32 x = __shfl_down(v[f], d); if (lane + d < nh) v[f] += x; }
	if (head && key >= 0 && (i64)key < nbin)
#pragma unroll
		for (int f = 0; f < 4; f++) if (v[f]) atomicAdd(bin + 4 * (i64)key + f, v[f]);
}

// the second level of a scan that leaves nothing but the total behind (a template: every pass's file is a translation unit of its own)
template <int = 0>
__global__ void __launch_bounds__(256) k_wg_total(i64 nwg, i64 *wg, i64 *total)
{
	__shared__ i64 s_w[4];
	const i64 t = wg_scan_sums(wg, nwg, s_w);
	if (threadIdx.x == 0) *total = t;
}

// the blocks of contig k in the final list (h_blocks[b0 .. b0 + nb)), where its records start, and where the contig starts in a bundle's concatenation
struct ResultRange { size_t b0, nb; i64 f0; i32 qoff; };
static inline ResultRange result_range(const gsa_ctx *c, i32 k)
{
	ResultRange r = { 0, c->h_blocks.size(), 0, 0 };
	if (!c->bnd.n) return r;
	if (c->h_blocks.empty() || c->b_nblk.size() != (size_t)c->bnd.n) { r.nb = 0; return r; }
	for (i32 j = 0; j < k; j++) r.b0 += (size_t)c->b_nblk[(size_t)j];
	r.nb = (size_t)c->b_nblk[(size_t)k]; r.f0 = c->b_frag0[(size_t)k]; r.qoff = c->b_off[(size_t)k];
	return r;
}

// ---- the span table (k_lift.hip, k_regions.hip as it stands; k_track.hip and k_proj.hip derive from it) ----
// One block with records: the text positions it covers [start, end) (end clamped to its chromosome copy), the greatest end of the entries up to this one (sorted tables
// only), its records (absolute), its first work item (ascending with the table), and what a choice between blocks and an answer need.  Entry [nt], where a pass asks
// for it: all zero but wbase = the work items
struct SpanBlk { i64 start, end, maxend, frag_off, wbase; i32 n_frag, rev, score, bdup, block, chr; };
struct SpanPick { i32 ent; uint16_t n_cover, _pad; };      // the chosen table entry (-1: no block covers the interval)
enum { SPAN_SORT = 1, SPAN_SENTINEL = 2 };

// The table of contig k's blocks into pinned `pin`, from the blocks and their first and last records, which the host holds: a few KB.  keep(block): the pass's filter
// (blocks without records never enter); extra(block, entry, first record, last record): the pass's own fields, non-zero fails the call.  SPAN_SORT: ordered by
// (start, block) with the running maximum of the ends; SPAN_SENTINEL: entry [nt].  nt entries, W records
template <class B, class Keep, class Extra>
static inline int span_build(gsa_ctx *c, const ResultRange &rr, const char *who, DevBuf &pin, int flags, Keep keep, Extra extra, i32 &nt, i64 &W)
{
	nt = 0; W = 0;
	if (!pin_ensure<B>(c, pin, rr.nb + 1)) return GSA_ERR_NOMEM;
	B *hb = (B *)pin.p;
	const gsa_rec *recs = c->p_frags.as<gsa_rec>() + rr.f0;
	for (size_t j = 0; j < rr.nb; j++) {
		const gsa_block &bl = c->h_blocks[rr.b0 + j];
		if (bl.n_frag <= 0 || !keep(bl)) continue;
		gsa_frag first, last;
		gsa_rec_expand(recs, bl.frag_off, &first); gsa_rec_expand(recs, bl.frag_off + bl.n_frag - 1, &last);
		const i64 fwd = c->h_chr_fwd[(size_t)bl.chr], len = c->h_chr_len[(size_t)bl.chr];
		const i64 lim = bl.bdir ? fwd + len : 2 * c->G - fwd;      // end of the block's chromosome copy (iExtension, tools.cpp:192-202)
		B &v = hb[nt];
		memset(&v, 0, sizeof(v));
		v.start = first.rpos; v.end = std::min<i64>(last.rpos + last.rlen, lim);
		if (v.end <= v.start) continue;
		v.frag_off = bl.frag_off + rr.f0; v.n_frag = bl.n_frag; v.rev = bl.bdir ? 0 : 1; v.score = bl.score; v.bdup = bl.bdup; v.block = (i32)j; v.chr = bl.chr;
		if (const int rc = extra(bl, v, first, last)) return rc;
		nt++;
	}
	if (flags & SPAN_SORT) std::sort(hb, hb + nt, [](const B &x, const B &y) { return x.start != y.start ? x.start < y.start : x.block < y.block; });
	for (i32 j = 0; j < nt; j++) { hb[j].maxend = j ? std::max(hb[j - 1].maxend, hb[j].end) : hb[j].end; hb[j].wbase = W; W += hb[j].n_frag; }
	if (W >= (1ll << 31) - 256) return gsa_fail(c, GSA_ERR_LIMIT, std::string(who) + ": too many records");
	if (flags & SPAN_SENTINEL) { memset(&hb[nt], 0, sizeof(B)); hb[nt].wbase = W; }
	return GSA_OK;
}

// (lift and regions: every block with records, no fields of their own)
static inline bool span_keep_all(const gsa_block &) { return true; }
static inline int span_no_extra(const gsa_block &, SpanBlk &, const gsa_frag &, const gsa_frag &) { return GSA_OK; }

// the choice between two blocks that overlap an interval by ox / oy bases: not a duplicate, then the greater overlap, then the greater score, then the smaller block index
__device__ __forceinline__ bool span_better(const SpanBlk &x, i64 ox, const SpanBlk &y, i64 oy)
{
	if ((x.bdup != 0) != (y.bdup != 0)) return x.bdup == 0;
	if (ox != oy) return ox > oy;
	if (x.score != y.score) return x.score > y.score;
	return x.block < y.block;
}

// the blocks of a SORTED table that overlap the text interval [lo, hi): a search for the last block that starts below hi and a scan backwards while the running maximum
// lies above lo; counted into n, the best of them (and of `best`, whose overlap is `bo`) into best
__device__ __forceinline__ void span_cover(const SpanBlk *blk, i32 nb, i64 lo, i64 hi, i32 &best, i64 &bo, u32 &n)
{
	if (blk[0].start >= hi) return;
	for (i32 j = blk_last_le(blk, nb, &SpanBlk::start, hi - 1); j >= 0 && blk[j].maxend > lo; j--) {
		const SpanBlk b = blk[j];
		if (b.end <= lo) continue;
		const i64 o = (b.end < hi ? b.end : hi) - (b.start > lo ? b.start : lo);
		n++;
		if (best < 0 || span_better(b, o, blk[best], bo)) { best = j; bo = o; }
	}
}

// the pick of the forward interval [beg, end): forward-strand blocks hold it as it stands, reverse-strand blocks as [2G - end, 2G - beg)
__device__ __forceinline__ SpanPick span_pick(const SpanBlk *blk, i32 nb, i64 G, i64 beg, i64 end)
{
	i32 best = -1; i64 bo = 0; u32 n = 0;
	span_cover(blk, nb, beg, end, best, bo, n);
	span_cover(blk, nb, 2 * G - end, 2 * G - beg, best, bo, n);
	SpanPick k; k.ent = best; k.n_cover = (uint16_t)(n > 65535u ? 65535u : n); k._pad = 0;
	return k;
}

// the last of records [lo, hi) with rpos <= t (record lo starts at or before t)
__device__ __forceinline__ i64 span_rec_of(const gsa_frag *frag, i64 lo, i64 hi, i64 t)
{
	while (hi - lo > 1) { const i64 m = (lo + hi) >> 1; if (frag[m].rpos <= t) lo = m; else hi = m; }
	return lo;
}

#endif
