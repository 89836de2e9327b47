// gsalign_amd/csrc/gsa_walk.h -- what the passes over a stage-8 result share (k_variants.hip, k_cigar.hip, k_cs.hip): the inputs of a
// record walk and the op string of a gap record, the search for the block of a work item, the two levels of the exclusive scan, and on the host the
// blocks of one contig of the result.  What a pass makes of a record -- which records it walks, what a column means -- stays with the pass.
#ifndef GSA_WALK_H
#define GSA_WALK_H
#include "gsa_ctx.h"
#include "gsa_gap.h"

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

// one block of the result, ALL of them, in result order: first record (absolute), records, strand, first work item; entry [nb]: wbase = W  (k_cigar.hip's
// block table d_cblk, read by k_cs.hip too)
struct CigBlk { i64 frag_off; i32 n_frag, bdir, wbase, _pad; };

// the last of t[0 .. n) whose key is <= x, 0 when there is none (entries that share a key -- blocks without records, without ops -- : the last of them)
template <class T, class K>
__device__ __forceinline__ i32 blk_last_le(const T *t, i32 n, K T::*key, i64 x)
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

#endif
