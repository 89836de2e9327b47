// gsalign_amd/csrc/k_qtrack.hip -- gsa_query_track: the per-window track of a stage-8 result over the QUERY contig (include/gsa_hip.h), on the device,
// over what stage 8 left there.  The mirror image of k_track.hip, and not a copy of it: one sequence and no chromosome grid; positions run forward on both strands
// (records hold contig positions as stored); the columns without a base of their own are the deletions; the trim is defined on the reference side and carried over; and
// a second interval table -- depth of at least two -- gives n_multi.
//
// Contig k is cut into windows of W bases; they stand in ONE dense array of {n_eq, n_x, n_ins, n_del} (16 bytes a window), which is all zero between calls.  The host
// builds small tables from the blocks and their end records, which it holds anyway: the counted blocks (gsa_walk.h's span table as it stands: bdup == 0, a valid chr,
// the clamped end), the blocks' kept query intervals [q0, q1) merged into disjoint depth >= 1 intervals, and the depth >= 2 intervals from a sweep over the sorted ends.
// q1 of a trimmed block is arithmetic where the cut falls into a seed or a pure deletion; where it falls into a gap, CUT counts the record's kept query bases:
//   CUT     (rare: a block that runs past the end of its chromosome copy inside a gap record) one wavefront per such record, 64 columns per step, until the first
//           column whose reference base is trimmed; the host waits for the answers, which the interval tables need
//   COUNT   one work item per record of the counted blocks.  A run record (a seed, a pure insertion) splits over the windows it spans by arithmetic, a pure deletion
//           charges one base, a gap is walked column by column.  A record that touches at most two windows is handled by its lane, and the lanes' counts are reduced
//           within the wavefront over runs of equal windows before ONE integer atomicAdd per (run, field) goes to the dense array (records ascend in query position
//           within a block); a record that touches more goes through the s_list / s_n queue to a wavefront: a run record 64 WINDOWS per step, a gap 64 COLUMNS per
//           step.  A 'D' column is charged to the query base in front of it: the step's query position carries that across the steps.
//   OWN     one work item per (depth >= 1 interval, window it touches); a window is owned by the first interval that touches it
//   SCAN    one workgroup turns the workgroups' sums into their first slots; the host reads the total and sizes the output
//   EMIT    the owners again: n_cov and n_multi are the window's overlaps with the two interval lists, the four counts are read from the dense array AND CLEARED there
// No workgroup waits for another, nothing spins; integer atomics only.  The columns of a DP gap come from the op string of its DP job (gsa_walk.h).
#include <vector>
#include "gsa_walk.h"

// one merged interval [s, e) of the contig under at least one counted block, sorted and disjoint; wbase: its first work item (one per window it touches).  Entry [niv]: wbase = items
struct QtkIv { i64 wbase; i32 s, e; };
struct QtkIv2 { i32 s, e; };                                  // the same under at least two, sorted and disjoint
struct QtkCut { i64 rec, end; };                              // a gap record (absolute) that holds its block's cut, and the cut
struct QtkIn : GapIn {
	const SpanBlk *blk; i32 nb; i64 n;                         // COUNT: the table and the work items
	const QtkIv *iv; i32 niv; i64 n_items;                     // OWN / EMIT
	const QtkIv2 *iv2; i32 niv2;
	i32 W, qoff, qlen; i64 nbin; u32 *bin;                     // start of the contig in a bundle's concatenation, its bases; the dense array: bin[4 window + {0 eq, 1 x, 2 ins, 3 del}]
	i64 n_out;
};

enum { QK_NONE = 0, QK_RUN = 1, QK_DEL = 2, QK_WALK = 3, QK_BAD = 4 };      // no kept column; n query bases of one class; n deleted bases behind query base q0; walked column by column; a DP record without a DP job
// what COUNT knows of a record before it looks at a column: the contig positions it may charge [q0, q1] and their two windows
struct QtkAt { i32 kind = QK_NONE, L = 0, f = 0, n = 0; const uint8_t *op = nullptr; i32 qpos = 0, qlen = 0, rlen = 0; i64 rpos = 0, end = 0; i32 q0 = 0, q1 = -1, wa = -1, wb = -1; bool bad = false; };

__device__ __forceinline__ QtkAt qtk_at(const QtkIn &a, i64 w)
{
	QtkAt x;
	const i32 bi = blk_last_le(a.blk, a.nb, &SpanBlk::wbase, w);
	const i64 i = a.blk[bi].frag_off + (w - a.blk[bi].wbase);
	x.end = a.blk[bi].end;
	const i32 t = a.ftype[i];
	const gsa_frag f = a.frag[i];
	x.qpos = f.qpos; x.qlen = f.qlen; x.rlen = f.rlen; x.rpos = f.rpos;
	const i32 q = f.qpos - a.qoff;
	const i64 left = x.end - f.rpos;                           // reference bases from the record's first that are kept
	if (t == FT_SEED) { if (f.qlen > 0 && left > 0) { x.kind = QK_RUN; x.f = 0; x.n = left < (i64)f.qlen ? (i32)left : f.qlen; x.q0 = q; x.q1 = q + x.n - 1; } }
	else if (f.qlen <= 0 && f.rlen <= 0) { }
	else if (f.qlen <= 0) { if (left > 0) { x.kind = QK_DEL; x.n = left < (i64)f.rlen ? (i32)left : f.rlen; x.q0 = x.q1 = q - 1; } }
	else if (f.rlen <= 0) { if (left >= 0) { x.kind = QK_RUN; x.f = 2; x.n = f.qlen; x.q0 = q; x.q1 = q + x.n - 1; } }      // (kept with the reference base in front of it)
	else if (left >= 0) {
		if (!gap_ops(a, i, t, f, x.op, x.L)) x.kind = QK_BAD;
		else if (x.L > 0) { x.kind = QK_WALK; x.q0 = q > 0 ? q - 1 : 0; x.q1 = q + f.qlen - 1; }      // (a leading 'D' column is charged to the base in front of the record)
	}
	if (x.kind == QK_NONE || x.kind == QK_BAD) return x;
	if (x.q0 < 0 || x.q1 < x.q0 || x.q1 >= a.qlen) { x.bad = true; x.kind = QK_NONE; return x; }
	x.wa = (i32)((u32)x.q0 / (u32)a.W); x.wb = (i32)((u32)x.q1 / (u32)a.W);
	return x;
}

// one column of a walked gap at (rp, qp), qp in the concatenation: whether it is kept, the field it counts in and the contig position it is charged to (-1 and
// beyond the contig: outside, reported by the caller)
__device__ __forceinline__ bool qtk_col(const QtkIn &a, i64 end, bool c1, bool c2, i64 rp, i32 qp, int &f, i32 &q)
{
	if (c1 ? rp >= end : rp > end) return false;
	f = !c1 ? 2 : (!c2 ? 3 : (int)col_mismatch(a.ref[rp], a.query[qp]));
	q = (c2 ? qp : qp - 1) - a.qoff;
	return true;
}

// a gap of at most WALK_SERIAL columns that touches the windows wa / wb only, by one lane; false: a column outside its record or the contig
__device__ bool qtk_lane(const QtkIn &a, const QtkAt &x, u32 vA[4], u32 vB[4])
{
	i64 rp = x.rpos; i32 qp = x.qpos;
	const i64 bnd = ((i64)x.wa + 1) * a.W;                     // first contig position of window wb
	for (i32 i = 0; i < x.L; i++) {
		const int ch = x.op ? (int)x.op[i] : (int)'M';
		const bool c1 = ch != 'D', c2 = ch != 'I';
		if ((c1 && rp - x.rpos >= x.rlen) || (c2 && qp - x.qpos >= x.qlen)) return false;
		int f; i32 q;
		if (!qtk_col(a, x.end, c1, c2, rp, qp, f, q)) return true;      // (the kept columns are a prefix)
		if (q < x.q0 || q > x.q1) return false;
		if ((i64)q < bnd) win_add(vA, f, 1u); else win_add(vB, f, 1u);
		col_advance(ch, rp, qp);
	}
	return rp - x.rpos == x.rlen && qp - x.qpos == x.qlen;
}

// the same by a whole wavefront, 64 columns per step (wave_step)
__device__ bool qtk_wave(const QtkIn &a, const QtkAt &x)
{
	i64 rp0 = x.rpos; i32 qp0 = x.qpos; bool ok = true, cut = false;
	for (i32 base = 0; base < x.L; base += 64) {
		const WaveCol w = wave_step(x.op, x.L, base, rp0, qp0);
		const bool out = (w.c1 && w.rp - x.rpos >= x.rlen) || (w.c2 && w.qp - x.qpos >= x.qlen);
		if (__ballot(out)) { ok = false; break; }
		u32 v[4] = { 0, 0, 0, 0 }; i32 key = -1;
		int f; i32 q;
		const bool kept = w.ch && qtk_col(a, x.end, w.c1, w.c2, w.rp, w.qp, f, q);
		if (kept) { if (q >= x.q0 && q <= x.q1) { key = (i32)((u32)q / (u32)a.W); win_add(v, f, 1u); } else ok = false; }
		win_flush(a.bin, a.nbin, key, v);
		if (__ballot(w.ch && !kept)) { cut = true; break; }      // (the kept columns are a prefix)
	}
	return __ballot(!ok) == 0ull && (cut || (rp0 - x.rpos == x.rlen && qp0 - x.qpos == x.qlen));
}

// a run record over more than two windows by a whole wavefront, 64 windows per step: every lane its own window, one atomic
__device__ void qtk_run_wave(const QtkIn &a, const QtkAt &x)
{
	const int lane = threadIdx.x & 63;
	for (i64 wn = (i64)x.wa + lane; wn <= (i64)x.wb; wn += 64) {
		const i64 lo = wn * (i64)a.W, hi = lo + a.W - 1;
		const i64 n = (hi < (i64)x.q1 ? hi : (i64)x.q1) - (lo > (i64)x.q0 ? lo : (i64)x.q0) + 1;
		if (n > 0 && wn < a.nbin) atomicAdd(a.bin + 4 * wn + x.f, (u32)n);
	}
}

// bad[0]: DP records without a DP job, bad[1]: columns outside their record or the contig -- neither can happen; both are counted and reported, never skipped silently
__global__ void __launch_bounds__(256) k_qtk_count(QtkIn a, unsigned long long *bad)
{
	__shared__ i32 s_list[256];
	__shared__ int s_n;
	const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
	const i64 w = (i64)blockIdx.x * 256 + tid;
	if (tid == 0) s_n = 0;
	__syncthreads();
	i32 kA = -1, kB = -1; u32 vA[4] = { 0, 0, 0, 0 }, vB[4] = { 0, 0, 0, 0 };
	if (w < a.n) {
		const QtkAt x = qtk_at(a, w);
		if (x.bad) atomicAdd(bad + 1, 1ull);
		if (x.kind == QK_BAD) atomicAdd(bad, 1ull);
		else if (x.kind == QK_NONE) { }
		else if (x.wb - x.wa > 1 || (x.kind == QK_WALK && x.L > WALK_SERIAL)) { const int at = atomicAdd(&s_n, 1); s_list[at] = tid; }
		else {
			kA = x.wa; if (x.wb != x.wa) kB = x.wb;
			if (x.kind == QK_DEL) vA[3] = (u32)x.n;
			else if (x.kind == QK_RUN) {
				const i64 nA = x.wb == x.wa ? (i64)x.n : ((i64)x.wa + 1) * a.W - x.q0;      // (the bases up to the first window's end)
				win_add(vA, x.f, (u32)nA); win_add(vB, x.f, (u32)(x.n - nA));
			}
			else if (!qtk_lane(a, x, vA, vB)) { atomicAdd(bad + 1, 1ull); kA = kB = -1; }
		}
	}
	win_flush(a.bin, a.nbin, kA, vA);
	win_flush(a.bin, a.nbin, kB, vB);
	__syncthreads();
	const int nlist = s_n;
	for (int q = wv; q < nlist; q += 4) {
		// (the record's look-up is repeated by every lane of the wavefront: the addresses are uniform, so the loads are one request each)
		const QtkAt x = qtk_at(a, (i64)blockIdx.x * 256 + s_list[q]);
		if (x.kind == QK_RUN) qtk_run_wave(a, x);
		else if (x.kind == QK_WALK) { if (!qtk_wave(a, x) && lane == 0) atomicAdd(bad + 1, 1ull); }
	}
}

// CUT: q1[i] = the contig position behind the last kept query base of gap record cut[i].rec, one wavefront per record (-1: a DP record without a DP job)
__global__ void __launch_bounds__(256) k_qtk_cut(QtkIn a, const QtkCut *cut, i32 ncut, i32 *q1)
{
	const int lane = threadIdx.x & 63;
	const i32 ci = (i32)blockIdx.x * 4 + (i32)(threadIdx.x >> 6);
	if (ci >= ncut) return;
	const i64 i = cut[ci].rec, end = cut[ci].end;
	const gsa_frag f = a.frag[i];
	const uint8_t *op = nullptr; i32 L = 0;
	if (!gap_ops(a, i, a.ftype[i], f, op, L)) { if (lane == 0) q1[ci] = -1; return; }
	i64 rp0 = f.rpos; i32 qp0 = f.qpos, q = f.qpos + f.qlen;
	for (i32 base = 0; base < L; base += 64) {
		const WaveCol w = wave_step(op, L, base, rp0, qp0);
		const unsigned long long m = __ballot(w.c1 && w.rp >= end);      // (the first trimmed reference base: every column in front of it is kept)
		if (m) { q = __shfl(w.qp, __ffsll((long long)m) - 1); break; }
	}
	if (lane == 0) q1[ci] = q - a.qoff;
}

// the window of EMIT work item w and whether its interval owns it
struct QtkItem { i32 iv, j; bool own; };
__device__ __forceinline__ QtkItem qtk_item(const QtkIn &a, i64 w)
{
	QtkItem x;
	x.iv = blk_last_le(a.iv, a.niv, &QtkIv::wbase, w);
	const QtkIv v = a.iv[x.iv];
	x.j = (i32)((u32)v.s / (u32)a.W) + (i32)(w - v.wbase);
	x.own = !(x.iv > 0 && (i32)((u32)(a.iv[x.iv - 1].e - 1) / (u32)a.W) == x.j);      // (sorted and disjoint: the predecessor alone decides)
	return x;
}

__global__ void __launch_bounds__(256) k_qtk_own(QtkIn a, i64 *wg)
{
	__shared__ i32 s_w[4];
	const i64 w = (i64)blockIdx.x * 256 + threadIdx.x;
	wg_count(w < a.n_items && qtk_item(a, w).own, s_w, wg);
}

__global__ void __launch_bounds__(256) k_qtk_scan(i64 nwg, i64 *wg, const unsigned long long *bad, i64 *hdr)
{
	__shared__ i64 s_w[4];
	const i64 total = wg_scan_sums(wg, nwg, s_w);
	if (threadIdx.x == 0) { hdr[0] = total; hdr[1] = (i64)bad[0]; hdr[2] = (i64)bad[1]; }
}

__global__ void __launch_bounds__(256) k_qtk_emit(QtkIn a, const i64 *wg, gsa_qtrack_win *out)
{
	__shared__ i32 s_w[4];
	const i64 w = (i64)blockIdx.x * 256 + threadIdx.x;
	QtkItem x; x.iv = 0; x.j = 0; x.own = false;
	if (w < a.n_items) x = qtk_item(a, w);
	const i64 slot = wg[blockIdx.x] + wg_excl_scan<i32>(x.own ? 1 : 0, s_w);
	if (!x.own) return;
	const i64 lo = (i64)x.j * a.W, hi = lo + a.W < (i64)a.qlen ? lo + a.W : (i64)a.qlen;      // the window [lo, hi)
	i64 cov = 0, multi = 0;
	for (i32 m = x.iv; m < a.niv; m++) {                // (the intervals that touch the window follow each other)
		const QtkIv u = a.iv[m];
		if ((i64)u.s >= hi) break;
		cov += ((i64)u.e < hi ? (i64)u.e : hi) - ((i64)u.s > lo ? (i64)u.s : lo);
	}
	if (a.niv2 > 0)
		for (i32 m = blk_last_le(a.iv2, a.niv2, &QtkIv2::s, lo); m < a.niv2; m++) {      // (from the last interval that starts at or below lo, or the first of all)
			const QtkIv2 u = a.iv2[m];
			if ((i64)u.s >= hi) break;
			const i64 o = ((i64)u.e < hi ? (i64)u.e : hi) - ((i64)u.s > lo ? (i64)u.s : lo);
			if (o > 0) multi += o;
		}
	uint4 c = make_uint4(0, 0, 0, 0);
	if ((i64)x.j < a.nbin) { uint4 *p = (uint4 *)a.bin + x.j; c = *p; *p = make_uint4(0, 0, 0, 0); }      // (read AND cleared: the dense array is all zero again when the pass ends)
	gsa_qtrack_win r;
	r.start = (int32_t)lo; r.len = (int32_t)(hi - lo); r.n_cov = (u32)cov; r.n_multi = (u32)multi; r.n_eq = c.x; r.n_x = c.y; r.n_ins = c.z; r.n_del = c.w;
	if (slot >= 0 && slot < a.n_out) out[slot] = r;
}

int query_track(gsa_ctx *c, i32 k, gsa_qtracks *out)
{
	const ResultRange rr = result_range(c, k);
	const i32 W = c->qtrack_w;
	const i32 qlen = c->bnd.n ? c->b_qlen[(size_t)k] : c->qlen;
	if (rr.nb == 0 || c->n_frags <= 0 || W <= 0 || qlen <= 0) return GSA_OK;
	if (!c->result_pinned) return gsa_fail(c, GSA_ERR_STATE, "gsa_query_track: the context holds no finished (stage 8) result");
	hipStream_t st = c->stream;
	const size_t nchr = c->h_chr_len.size();
	if (!pin_ensure<i64>(c, c->p_qhdr, 4)) return GSA_ERR_NOMEM;
	// the counted blocks (not duplicates, on a sequence the index knows: gsa_ref_track's set) with their clamped ends -- the span table as it stands -- and beside it, on
	// the host only, the query interval [q0, q1) of every entry (entries keep the blocks' order: no sort)
	struct QSpan { i32 q0, q1; bool trimmed; };
	std::vector<QSpan> qs;
	i32 nt = 0; i64 items = 0; unsigned long long depth = 0;
	auto keep = [&](const gsa_block &bl) { return bl.bdup == 0 && bl.chr >= 0 && (size_t)bl.chr < nchr; };
	auto extra = [&](const gsa_block &, SpanBlk &v, const gsa_frag &first, const gsa_frag &last) {
		depth += (unsigned long long)(last.rpos + last.rlen - first.rpos) + (unsigned long long)std::max<i64>((i64)last.qpos + last.qlen - first.qpos, 0);
		QSpan s; s.q0 = first.qpos; s.q1 = last.qpos + last.qlen; s.trimmed = last.rpos + last.rlen > v.end;
		if (s.q0 < 0 || s.q1 > qlen) return gsa_fail(c, GSA_ERR_STATE, "internal: gsa_query_track met a block outside its contig");
		qs.push_back(s);
		return (int)GSA_OK;
	};
	if (const int rc = span_build<SpanBlk>(c, rr, "gsa_query_track", c->p_qblk, SPAN_SENTINEL, keep, extra, nt, items)) return rc;
	if (nt == 0) return GSA_OK;
	// (the counts are uint32_t, and none can exceed the columns of the counted blocks: include/gsa_hip.h)
	if (depth > 0xffffffffull) return gsa_fail(c, GSA_ERR_LIMIT, "gsa_query_track: the counted blocks span " + std::to_string(depth) + " bases, more than a 32-bit count holds");
	QtkIn a;
	gap_in_fill(c, a);
	ENS(SpanBlk, d_qblk, (size_t)nt + 1);
	GSA_CHECK(c, hipMemcpyAsync(c->d_qblk.p, c->p_qblk.p, ((size_t)nt + 1) * sizeof(SpanBlk), hipMemcpyHostToDevice, st));
	a.blk = c->d_qblk.as<SpanBlk>(); a.nb = nt; a.n = items; a.iv = nullptr; a.niv = 0; a.n_items = 0; a.iv2 = nullptr; a.niv2 = 0;
	a.W = W; a.qoff = rr.qoff; a.qlen = qlen; a.nbin = 0; a.bin = nullptr; a.n_out = 0;
	// q1 of a trimmed block: the record that holds the first trimmed reference base (the records' ends ascend) -- arithmetic in a seed or a pure deletion, CUT in a gap
	{
		const SpanBlk *hb = c->p_qblk.as<SpanBlk>();
		const gsa_rec *recs = c->p_frags.as<gsa_rec>();
		std::vector<QtkCut> cuts; std::vector<i32> cut_of;
		for (i32 j = 0; j < nt; j++) {
			if (!qs[(size_t)j].trimmed) continue;
			i64 lo = 0, hi = hb[j].n_frag;      // the first record of the block with rpos + rlen > end
			gsa_frag f;
			while (lo < hi) { const i64 m = (lo + hi) >> 1; gsa_rec_expand(recs, hb[j].frag_off + m, &f); if (f.rpos + f.rlen > hb[j].end) hi = m; else lo = m + 1; }
			if (lo >= hb[j].n_frag) continue;
			gsa_rec_expand(recs, hb[j].frag_off + lo, &f);
			if (f.bseed) qs[(size_t)j].q1 = f.qpos + (i32)std::max<i64>(hb[j].end - f.rpos, 0);
			else if (f.qlen <= 0 || hb[j].end < f.rpos) qs[(size_t)j].q1 = f.qpos;
			else { QtkCut u; u.rec = hb[j].frag_off + lo; u.end = hb[j].end; cuts.push_back(u); cut_of.push_back(j); }
		}
		if (!cuts.empty()) {
			const size_t nc = cuts.size(), bytes = nc * (sizeof(QtkCut) + sizeof(i32));
			if (!pin_ensure<uint8_t>(c, c->p_qcut, bytes)) return GSA_ERR_NOMEM;
			ENS(uint8_t, d_qcut, bytes);
			memcpy(c->p_qcut.p, cuts.data(), nc * sizeof(QtkCut));
			i32 *hq = (i32 *)((uint8_t *)c->p_qcut.p + nc * sizeof(QtkCut)), *dq = (i32 *)((uint8_t *)c->d_qcut.p + nc * sizeof(QtkCut));
			GSA_CHECK(c, hipMemcpyAsync(c->d_qcut.p, c->p_qcut.p, nc * sizeof(QtkCut), hipMemcpyHostToDevice, st));
			hipLaunchKernelGGL(k_qtk_cut, dim3((unsigned)((nc + 3) / 4)), dim3(256), 0, st, a, (const QtkCut *)c->d_qcut.p, (i32)nc, dq);
			GSA_CHECK(c, hipGetLastError());
			GSA_CHECK(c, hipMemcpyAsync(hq, dq, nc * sizeof(i32), hipMemcpyDeviceToHost, st));
			GSA_CHECK(c, hipStreamSynchronize(st));
			for (size_t i = 0; i < nc; i++) {
				QSpan &s = qs[(size_t)cut_of[i]];
				if (hq[i] < 0) return gsa_fail(c, GSA_ERR_STATE, "internal: gsa_query_track met a DP record without a DP job");
				if (hq[i] < s.q0 || hq[i] > s.q1) return gsa_fail(c, GSA_ERR_STATE, "internal: gsa_query_track met a cut outside its block");
				s.q1 = hq[i];
			}
		}
	}
	// the depth >= 1 intervals (sorted, merged) and, from a sweep over the sorted ends, the depth >= 2 intervals
	std::vector<QtkIv> iv; std::vector<QtkIv2> iv2;
	{
		std::vector<std::pair<i32, i32> > ev;      // (position, -1 / +1): an end sorts in front of a start at the same position, so blocks that merely touch are not depth 2
		for (const QSpan &s : qs) if (s.q1 > s.q0) { QtkIv u; u.wbase = 0; u.s = s.q0; u.e = s.q1; iv.push_back(u); ev.push_back({ s.q0, 1 }); ev.push_back({ s.q1, -1 }); }
		if (iv.empty()) return GSA_OK;
		std::sort(iv.begin(), iv.end(), [](const QtkIv &x, const QtkIv &y) { return x.s != y.s ? x.s < y.s : x.e < y.e; });
		size_t n1 = 0;
		for (size_t j = 0; j < iv.size(); j++) {
			if (n1 && iv[j].s <= iv[n1 - 1].e) iv[n1 - 1].e = std::max(iv[n1 - 1].e, iv[j].e);
			else iv[n1++] = iv[j];
		}
		iv.resize(n1);
		std::sort(ev.begin(), ev.end());
		i32 d = 0;
		for (const auto &e : ev) {
			const i32 was = d; d += e.second;
			if (was == 1 && d == 2) { if (!iv2.empty() && iv2.back().e == e.first) iv2.back().e = -1; else { QtkIv2 u; u.s = e.first; u.e = -1; iv2.push_back(u); } }
			else if (was == 2 && d == 1) iv2.back().e = e.first;
		}
	}
	const size_t niv = iv.size(), niv2 = iv2.size();
	i64 n_items = 0;
	for (size_t j = 0; j < niv; j++) { iv[j].wbase = n_items; n_items += (i64)((iv[j].e - 1) / W - iv[j].s / W + 1); }
	if (n_items >= (1ll << 31) - 256) return gsa_fail(c, GSA_ERR_LIMIT, "gsa_query_track: too many windows");
	// (one pinned and one device buffer for both interval lists: the depth >= 1 intervals with their sentinel, then the depth >= 2 intervals)
	const size_t iv_bytes = (niv + 1) * sizeof(QtkIv), iv2_bytes = (niv2 + 1) * sizeof(QtkIv2);
	if (!pin_ensure<uint8_t>(c, c->p_qiv, iv_bytes + iv2_bytes)) return GSA_ERR_NOMEM;
	{
		QtkIv *hv = (QtkIv *)c->p_qiv.p;
		memcpy(hv, iv.data(), niv * sizeof(QtkIv));
		memset(&hv[niv], 0, sizeof(QtkIv)); hv[niv].wbase = n_items;
		memset((uint8_t *)c->p_qiv.p + iv_bytes, 0, iv2_bytes);
		if (niv2) memcpy((uint8_t *)c->p_qiv.p + iv_bytes, iv2.data(), niv2 * sizeof(QtkIv2));
	}
	const i64 nbin = ((i64)qlen + W - 1) / W;
	const i64 nwg_c = (items + 255) / 256, nwg_e = (n_items + 255) / 256;
	ENS(uint8_t, d_qiv, iv_bytes + iv2_bytes); ENS(i64, d_qwg, (size_t)nwg_e + 2);      // sums | {records without a job, columns outside their record}
	// the dense array: grown to the longest contig seen, cleared once -- a call that grew it, or one that failed between COUNT and EMIT, clears it again
	{
		const size_t had = c->d_qbin.cap;
		ENS(uint4, d_qbin, (size_t)nbin);
		if (c->d_qbin.cap != had) c->qtrack_zeroed = 0;
		if (c->qtrack_dirty || c->qtrack_zeroed < (size_t)nbin) {
			GSA_CHECK(c, hipMemsetAsync(c->d_qbin.p, 0, (size_t)nbin * sizeof(uint4), st));
			// (only [0, nbin) is cleared, and qtrack_zeroed is LOWERED to nbin with it: what a failed larger call left beyond nbin is cleared by the next call that reaches there)
			c->qtrack_zeroed = (size_t)nbin; c->qtrack_dirty = false;
		}
	}
	i64 *wg = c->d_qwg.as<i64>(); unsigned long long *bad = (unsigned long long *)(wg + nwg_e);
	i64 *hdr = c->p_qhdr.as<i64>();
	GSA_CHECK(c, hipMemcpyAsync(c->d_qiv.p, c->p_qiv.p, iv_bytes + iv2_bytes, hipMemcpyHostToDevice, st));
	GSA_CHECK(c, hipMemsetAsync(bad, 0, 2 * sizeof(unsigned long long), st));
	a.iv = (const QtkIv *)c->d_qiv.p; a.niv = (i32)niv; a.n_items = n_items; a.iv2 = (const QtkIv2 *)((const uint8_t *)c->d_qiv.p + iv_bytes); a.niv2 = (i32)niv2;
	a.nbin = nbin; a.bin = c->d_qbin.as<u32>();
	c->qtrack_dirty = true;      // (until EMIT has run)
	hipLaunchKernelGGL(k_qtk_count, dim3((unsigned)nwg_c), dim3(256), 0, st, a, bad);
	GSA_CHECK(c, hipGetLastError());
	hipLaunchKernelGGL(k_qtk_own, dim3((unsigned)nwg_e), dim3(256), 0, st, a, wg);
	GSA_CHECK(c, hipGetLastError());
	hipLaunchKernelGGL(k_qtk_scan, dim3(1), dim3(256), 0, st, nwg_e, wg, (const unsigned long long *)bad, hdr);
	GSA_CHECK(c, hipGetLastError());
	GSA_CHECK(c, hipStreamSynchronize(st));
	const i64 nw = hdr[0];
	if (hdr[1]) return gsa_fail(c, GSA_ERR_STATE, "internal: gsa_query_track met " + std::to_string((long long)hdr[1]) + " DP record(s) without a DP job");
	if (hdr[2]) return gsa_fail(c, GSA_ERR_STATE, "internal: gsa_query_track met " + std::to_string((long long)hdr[2]) + " column(s) outside the record or contig that should hold them");
	if (nw <= 0 || nw > n_items) return gsa_fail(c, GSA_ERR_STATE, "internal: gsa_query_track counted more windows than the intervals touch");
	// the output is sized from the scan's total; it goes home in one copy
	ENS(gsa_qtrack_win, d_qout, (size_t)nw); if (!pin_ensure<gsa_qtrack_win>(c, c->p_qout, (size_t)nw)) return GSA_ERR_NOMEM;
	a.n_out = nw;
	hipLaunchKernelGGL(k_qtk_emit, dim3((unsigned)nwg_e), dim3(256), 0, st, a, (const i64 *)wg, c->d_qout.as<gsa_qtrack_win>());
	GSA_CHECK(c, hipGetLastError());
	GSA_CHECK(c, hipMemcpyAsync(c->p_qout.p, c->d_qout.p, (size_t)nw * sizeof(gsa_qtrack_win), hipMemcpyDeviceToHost, st));
	GSA_CHECK(c, hipStreamSynchronize(st));
	c->qtrack_dirty = false;
	out->n_win = nw; out->win = c->p_qout.as<gsa_qtrack_win>();
	return GSA_OK;
}
