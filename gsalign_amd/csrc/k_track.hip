// gsalign_amd/csrc/k_track.hip -- gsa_ref_track: the per-window track of a stage-8 result over the reference sequences (include/gsa_hip.h), on the
// device, over what stage 8 left there.
//
// The reference sequences are cut into windows of W bases, the grid restarting at every sequence; the windows of all sequences stand in ONE dense array of
// {n_eq, n_x, n_del, n_ins} (16 bytes a window), which is all zero between calls.  The host builds two small tables from the blocks and their end records, which it
// holds anyway: the counted blocks (bdup == 0) with their records and their trimmed spans, and those spans mapped to forward coordinates and merged into disjoint
// intervals per sequence.
//   COUNT   one work item per record of the counted blocks.  A run record (a seed, a pure deletion) splits over the windows it spans by arithmetic; a gap is walked
//           column by column.  A record that touches at most two windows is handled by its lane, and the lanes' counts are reduced within the wavefront over runs of
//           equal windows before ONE integer atomicAdd per (run, field) goes to the dense array (records ascend in text position, so neighbouring lanes hit the same
//           or the next window); a record that touches more goes through the s_list / s_n queue to a wavefront: a run record 64 WINDOWS per step (distinct windows,
//           one atomic each), a gap 64 COLUMNS per step with ballot / popcount and the same reduction.  Integer atomics: any order gives the same sums.
//   OWN     one work item per (interval, window it touches); a window is owned by the first interval that touches it -- the intervals are sorted and disjoint, so the
//           predecessor alone decides -- and the owners are counted per workgroup
//   SCAN    one workgroup turns the workgroups' sums into their first slots; the host reads the total and sizes the output
//   EMIT    the owners again: n_cov is the window's overlap with the intervals, the four counts are read from the dense array AND CLEARED there, the record goes to its
//           slot, so the windows are dense and ascend by (chr, start)
// No workgroup waits for another, nothing spins.  As in the other passes the columns of a DP gap come from the op string of its DP job (gsa_walk.h), never from the
// string pools.
#include <vector>
#include "gsa_walk.h"

// one counted block with records (gsa_walk.h's span table entry, unsorted) and the way from a text position t to a window: local = rev ? org - t : t - org inside the
// block's sequence of clen bases, window win0 + local / W.  Entry [nb]: wbase = items.  Padded to 128 bytes: with a power-of-two stride the searches index by a shift,
// which keeps k_trk_count at the 64 registers it had with its own 56-byte entry (80 bytes unpadded: 66, a wave per SIMD less; the table is a few KB either way)
struct TrkBlk : SpanBlk { i64 org; i32 win0, clen; i64 _pad[6]; };
// one merged interval [s, e) of covered forward positions inside sequence chr (clen bases, first window win0), sorted by (chr, s) and disjoint; wbase: its first work
// item (one per window it touches).  Entry [niv]: wbase = items
struct TrkIv { i64 wbase; i32 chr, s, e, clen, win0, _pad; };
struct TrkIn : GapIn {
	const TrkBlk *blk; i32 nb; i64 n;                          // COUNT: the table and the work items
	const TrkIv *iv; i32 niv; i64 n_items;                     // OWN / EMIT
	i32 W; i64 nbin; u32 *bin;                                 // the dense array: bin[4 window + {0 eq, 1 x, 2 del, 3 ins}]
	i64 n_out;
};

enum { TK_NONE = 0, TK_RUN = 1, TK_INS = 2, TK_WALK = 3, TK_BAD = 4 };      // no covered column; rlen reference bases of one class; qlen inserted bases behind rpos - 1; walked column by column; a DP record without a DP job
struct TrkRec { i32 kind = TK_NONE, L = 0, f = 0; const uint8_t *op = nullptr; i32 qpos = 0, qlen = 0, rlen = 0; i64 rpos = 0; };

__device__ __forceinline__ TrkRec trk_load(const TrkIn &a, i64 i)
{
	TrkRec g;
	const i32 t = a.ftype[i];
	const gsa_frag f = a.frag[i];
	g.qpos = f.qpos; g.qlen = f.qlen; g.rlen = f.rlen; g.rpos = f.rpos;
	if (t == FT_SEED) { if (f.rlen > 0) { g.kind = TK_RUN; g.f = 0; } return g; }
	if (f.qlen <= 0 && f.rlen <= 0) return g;
	if (f.qlen <= 0) { g.kind = TK_RUN; g.f = 2; return g; }
	if (f.rlen <= 0) { g.kind = TK_INS; return g; }
	if (!gap_ops(a, i, t, f, g.op, g.L)) g.kind = TK_BAD;
	else if (g.L > 0) g.kind = TK_WALK;
	return g;
}

// the window of text position t of block b; -1: outside the block's sequence (cannot happen for a covered position; reported)
__device__ __forceinline__ i32 trk_win(const TrkIn &a, const TrkBlk &b, i64 t)
{
	const i64 l = b.rev ? b.org - t : t - b.org;
	if (l < 0 || l >= (i64)b.clen) return -1;
	const i64 w = (i64)b.win0 + (i64)((u32)l / (u32)a.W);
	return w < a.nbin ? (i32)w : -1;
}

// (the lanes' counts into the dense array: gsa_walk.h's win_add / win_flush, which k_qtrack.hip shares)
__device__ __forceinline__ void trk_add(u32 v[4], int f, u32 n) { win_add(v, f, n); }
__device__ __forceinline__ void trk_flush(const TrkIn &a, i32 key, u32 v[4]) { win_flush(a.bin, a.nbin, key, v); }

// what COUNT knows of a record before it looks at a column: the covered text positions it may charge [t0, t1] (for a gap with rpos - 1 in front, where a leading
// insertion belongs) and their two windows
struct TrkAt { TrkRec g; TrkBlk b; i64 t0 = 0, t1 = -1; i32 wa = -1, wb = -1; bool bad = false; };

__device__ __forceinline__ TrkAt trk_at(const TrkIn &a, i64 w)
{
	TrkAt x;
	const i32 bi = blk_last_le(a.blk, a.nb, &TrkBlk::wbase, w);
	x.b = a.blk[bi];
	x.g = trk_load(a, x.b.frag_off + (w - x.b.wbase));
	if (x.g.kind == TK_NONE || x.g.kind == TK_BAD) return x;
	x.t0 = x.g.kind == TK_RUN ? x.g.rpos : x.g.rpos - 1;
	x.t1 = x.g.kind == TK_INS ? x.g.rpos - 1 : x.g.rpos + x.g.rlen - 1;
	if (x.t0 < x.b.start) x.t0 = x.b.start;
	if (x.t1 >= x.b.end) x.t1 = x.b.end - 1;
	if (x.t1 < x.t0) { x.g.kind = TK_NONE; return x; }       // (everything the record could charge is trimmed)
	x.wa = trk_win(a, x.b, x.t0); x.wb = trk_win(a, x.b, x.t1);
	if (x.wa < 0 || x.wb < 0) { x.bad = true; x.g.kind = TK_NONE; }
	return x;
}

// one column of a walked gap: the field it counts in ('M': 0 '=' until the caller has compared the two bases -- they are read for counted columns only) and the text
// position it is charged to; false: no count (trimmed)
__device__ __forceinline__ bool trk_col(const TrkBlk &b, int ch, i64 rp, int &f, i64 &t)
{
	if (ch == 'D') { f = 3; t = rp - 1; }             // ('D' puts '-' into the reference row: CIGAR I, charged to the base consumed last)
	else { f = ch == 'I' ? 2 : 0; t = rp; }
	return t >= b.start && t < b.end;
}

// a gap of at most WALK_SERIAL columns that touches the windows wa / wb only, by one lane; false: a column outside its record
__device__ bool trk_lane(const TrkIn &a, const TrkAt &x, u32 vA[4], u32 vB[4])
{
	const TrkRec &g = x.g;
	i64 rp = g.rpos; i32 qp = g.qpos;
	for (i32 i = 0; i < g.L; i++) {
		const int ch = g.op ? (int)g.op[i] : (int)'M';
		if ((ch != 'D' && rp - g.rpos >= g.rlen) || (ch != 'I' && qp - g.qpos >= g.qlen)) return false;
		int f; i64 t;
		if (trk_col(x.b, ch, rp, f, t)) { if (ch == 'M') f = (int)col_mismatch(a.ref[rp], a.query[qp]); if (trk_win(a, x.b, t) == x.wa) trk_add(vA, f, 1u); else trk_add(vB, f, 1u); }
		col_advance(ch, rp, qp);
	}
	return rp - g.rpos == g.rlen && qp - g.qpos == g.qlen;
}

// the same by a whole wavefront, 64 columns per step (wave_step)
__device__ bool trk_wave(const TrkIn &a, const TrkAt &x)
{
	const TrkRec &g = x.g;
	i64 rp0 = g.rpos; i32 qp0 = g.qpos; bool ok = true;
	for (i32 base = 0; base < g.L; base += 64) {
		const WaveCol w = wave_step(g.op, g.L, base, rp0, qp0);
		const bool out = (w.c1 && w.rp - g.rpos >= g.rlen) || (w.c2 && w.qp - g.qpos >= g.qlen);
		if (__ballot(out)) { ok = false; break; }
		u32 v[4] = { 0, 0, 0, 0 }; i32 key = -1;
		int f; i64 t;
		if (w.ch && trk_col(x.b, w.ch, w.rp, f, t)) { if (w.ch == 'M') f = (int)col_mismatch(a.ref[w.rp], a.query[w.qp]); key = trk_win(a, x.b, t); if (key >= 0) trk_add(v, f, 1u); else ok = false; }
		trk_flush(a, key, v);
	}
	return __ballot(!ok) == 0ull && rp0 - g.rpos == g.rlen && qp0 - g.qpos == g.qlen;
}

// a run record over more than two windows by a whole wavefront, 64 windows per step: every lane its own window, one atomic
__device__ void trk_run_wave(const TrkIn &a, const TrkAt &x)
{
	const int lane = threadIdx.x & 63;
	const TrkBlk &b = x.b;
	const i64 l0 = b.rev ? b.org - x.t1 : x.t0 - b.org, l1 = b.rev ? b.org - x.t0 : x.t1 - b.org;      // the run's local positions [l0, l1]
	const i32 w0 = x.wa < x.wb ? x.wa : x.wb, w1 = x.wa < x.wb ? x.wb : x.wa;
	for (i64 wn = (i64)w0 + lane; wn <= (i64)w1; wn += 64) {
		const i64 lo = (wn - b.win0) * (i64)a.W, hi = lo + a.W - 1;
		const i64 n = (hi < l1 ? hi : l1) - (lo > l0 ? lo : l0) + 1;
		if (n > 0 && wn < a.nbin) atomicAdd(a.bin + 4 * wn + x.g.f, (u32)n);
	}
}

// bad[0]: DP records without a DP job, bad[1]: columns outside their record or their sequence -- neither can happen; both are counted and reported, never skipped silently
__global__ void __launch_bounds__(256) k_trk_count(TrkIn a, unsigned long long *bad)
{
	__shared__ i32 s_list[256];
	__shared__ int s_n;
	const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
	const i64 w = (i64)blockIdx.x * 256 + tid;
	if (tid == 0) s_n = 0;
	__syncthreads();
	i32 kA = -1, kB = -1; u32 vA[4] = { 0, 0, 0, 0 }, vB[4] = { 0, 0, 0, 0 };
	if (w < a.n) {
		const TrkAt x = trk_at(a, w);
		const TrkRec &g = x.g;
		const i32 span = x.wa < x.wb ? x.wb - x.wa : x.wa - x.wb;
		if (x.bad) atomicAdd(bad + 1, 1ull);
		if (g.kind == TK_BAD) atomicAdd(bad, 1ull);
		else if (g.kind == TK_NONE) { }
		else if (span > 1 || (g.kind == TK_WALK && g.L > WALK_SERIAL)) { const int at = atomicAdd(&s_n, 1); s_list[at] = tid; }
		else {
			kA = x.wa; if (x.wb != x.wa) kB = x.wb;
			if (g.kind == TK_INS) vA[3] = (u32)g.qlen;
			else if (g.kind == TK_RUN) {
				// (the bases of the first window: up to its end for a forward block, down to its start for a reverse-strand block)
				const i64 n = x.t1 - x.t0 + 1, l = x.b.rev ? x.b.org - x.t0 : x.t0 - x.b.org, j = (i64)(x.wa - x.b.win0) * a.W;
				const i64 nA = x.wb == x.wa ? n : (x.b.rev ? l - j + 1 : j + a.W - l);
				trk_add(vA, g.f, (u32)nA); trk_add(vB, g.f, (u32)(n - nA));
			}
			else if (!trk_lane(a, x, vA, vB)) { atomicAdd(bad + 1, 1ull); kA = kB = -1; }
		}
	}
	trk_flush(a, kA, vA);
	trk_flush(a, kB, vB);
	__syncthreads();
	const int nlist = s_n;
	for (int q = wv; q < nlist; q += 4) {
		// (the record's look-up is repeated by every lane of the wavefront: the addresses are uniform, so the loads are one request each)
		const TrkAt x = trk_at(a, (i64)blockIdx.x * 256 + s_list[q]);
		if (x.g.kind == TK_RUN) trk_run_wave(a, x);
		else if (x.g.kind == TK_WALK) { if (!trk_wave(a, x) && lane == 0) atomicAdd(bad + 1, 1ull); }
	}
}

// the window of EMIT work item w and whether its interval owns it
struct TrkItem { i32 iv, j; bool own; };
__device__ __forceinline__ TrkItem trk_item(const TrkIn &a, i64 w)
{
	TrkItem x;
	x.iv = blk_last_le(a.iv, a.niv, &TrkIv::wbase, w);
	const TrkIv v = a.iv[x.iv];
	x.j = (i32)((u32)v.s / (u32)a.W) + (i32)(w - v.wbase);
	x.own = true;
	if (x.iv > 0) { const TrkIv p = a.iv[x.iv - 1]; if (p.chr == v.chr && (i32)((u32)(p.e - 1) / (u32)a.W) == x.j) x.own = false; }
	return x;
}

__global__ void __launch_bounds__(256) k_trk_own(TrkIn a, i64 *wg)
{
	__shared__ i32 s_w[4];
	const i64 w = (i64)blockIdx.x * 256 + threadIdx.x;
	wg_count(w < a.n_items && trk_item(a, w).own, s_w, wg);
}

__global__ void __launch_bounds__(256) k_trk_scan(i64 nwg, i64 *wg, const unsigned long long *bad, i64 *hdr)
{
	__shared__ i64 s_w[4];
	const i64 total = wg_scan_sums(wg, nwg, s_w);
	if (threadIdx.x == 0) { hdr[0] = total; hdr[1] = (i64)bad[0]; hdr[2] = (i64)bad[1]; }
}

__global__ void __launch_bounds__(256) k_trk_emit(TrkIn a, const i64 *wg, gsa_track_win *out)
{
	__shared__ i32 s_w[4];
	const i64 w = (i64)blockIdx.x * 256 + threadIdx.x;
	TrkItem x; x.iv = 0; x.j = 0; x.own = false;
	if (w < a.n_items) x = trk_item(a, w);
	const i64 slot = wg[blockIdx.x] + wg_excl_scan<i32>(x.own ? 1 : 0, s_w);
	if (!x.own) return;
	const TrkIv v = a.iv[x.iv];
	const i64 lo = (i64)x.j * a.W, hi = lo + a.W < (i64)v.clen ? lo + a.W : (i64)v.clen;      // the window [lo, hi)
	i64 cov = 0;
	for (i32 m = x.iv; m < a.niv; m++) {                // (the intervals that touch the window follow each other)
		const TrkIv u = a.iv[m];
		if (u.chr != v.chr || (i64)u.s >= hi) break;
		cov += ((i64)u.e < hi ? (i64)u.e : hi) - ((i64)u.s > lo ? (i64)u.s : lo);
	}
	const i64 bi = (i64)v.win0 + x.j;
	uint4 c = make_uint4(0, 0, 0, 0);
	if (bi >= 0 && bi < a.nbin) { uint4 *p = (uint4 *)a.bin + bi; c = *p; *p = make_uint4(0, 0, 0, 0); }      // (read AND cleared: the dense array is all zero again when the pass ends)
	gsa_track_win r;
	r.chr = v.chr; r.start = (int32_t)lo; r.len = (int32_t)(hi - lo); r.n_cov = (u32)cov; r.n_eq = c.x; r.n_x = c.y; r.n_del = c.z; r.n_ins = c.w;
	if (slot >= 0 && slot < a.n_out) out[slot] = r;
}

int ref_track(gsa_ctx *c, i32 k, gsa_tracks *out)
{
	const ResultRange rr = result_range(c, k);
	const size_t nb = rr.nb;
	const i32 W = c->track_w;
	if (nb == 0 || c->n_frags <= 0 || W <= 0) return GSA_OK;
	if (!c->result_pinned) return gsa_fail(c, GSA_ERR_STATE, "gsa_ref_track: the context holds no finished (stage 8) result");
	hipStream_t st = c->stream;
	const size_t nchr = c->h_chr_len.size();
	if (!pin_ensure<i64>(c, c->p_thdr, 4)) return GSA_ERR_NOMEM;
	std::vector<i32> win0(nchr + 1, 0);
	for (size_t i = 0; i < nchr; i++) win0[i + 1] = win0[i] + (i32)(((i64)c->h_chr_len[i] + W - 1) / W);
	// the counted blocks (not duplicates, on a sequence the index knows), and their trimmed spans in forward coordinates
	i32 nt = 0; i64 items = 0; unsigned long long depth = 0;
	std::vector<TrkIv> iv;
	auto keep = [&](const gsa_block &bl) { return bl.bdup == 0 && bl.chr >= 0 && (size_t)bl.chr < nchr; };
	auto extra = [&](const gsa_block &bl, TrkBlk &v, const gsa_frag &first, const gsa_frag &last) {
		const i64 fwd = c->h_chr_fwd[(size_t)bl.chr], len = c->h_chr_len[(size_t)bl.chr];
		v.org = v.rev ? 2 * c->G - 1 - fwd : fwd; v.win0 = win0[(size_t)bl.chr]; v.clen = (i32)len;
		const i64 s = v.rev ? v.org - (v.end - 1) : v.start - v.org, e = v.rev ? v.org - v.start + 1 : v.end - v.org;      // [s, e) inside the sequence
		if (s < 0 || e > len) return gsa_fail(c, GSA_ERR_STATE, "internal: gsa_ref_track met a block outside its reference sequence");
		depth += (unsigned long long)(last.rpos + last.rlen - first.rpos) + (unsigned long long)std::max<i64>((i64)last.qpos + last.qlen - first.qpos, 0);
		TrkIv u; u.wbase = 0; u.chr = bl.chr; u.s = (i32)s; u.e = (i32)e; u.clen = (i32)len; u.win0 = v.win0; u._pad = 0;
		iv.push_back(u);
		return (int)GSA_OK;
	};
	if (const int rc = span_build<TrkBlk>(c, rr, "gsa_ref_track", c->p_tblk, SPAN_SENTINEL, keep, extra, nt, items)) return rc;
	if (nt == 0) return GSA_OK;
	// (the counts are uint32_t, and none can exceed the columns of the counted blocks: include/gsa_hip.h)
	if (depth > 0xffffffffull) return gsa_fail(c, GSA_ERR_LIMIT, "gsa_ref_track: the counted blocks span " + std::to_string(depth) + " bases, more than a 32-bit count holds");
	std::sort(iv.begin(), iv.end(), [](const TrkIv &x, const TrkIv &y) { return x.chr != y.chr ? x.chr < y.chr : (x.s != y.s ? x.s < y.s : x.e < y.e); });
	size_t niv = 0;
	for (size_t j = 0; j < iv.size(); j++) {
		if (niv && iv[niv - 1].chr == iv[j].chr && iv[j].s <= iv[niv - 1].e) iv[niv - 1].e = std::max(iv[niv - 1].e, iv[j].e);
		else iv[niv++] = iv[j];
	}
	i64 n_items = 0;
	for (size_t j = 0; j < niv; j++) { iv[j].wbase = n_items; n_items += (i64)((iv[j].e - 1) / W - iv[j].s / W + 1); }
	if (n_items >= (1ll << 31) - 256) return gsa_fail(c, GSA_ERR_LIMIT, "gsa_ref_track: too many windows");
	if (!pin_ensure<TrkIv>(c, c->p_tiv, niv + 1)) return GSA_ERR_NOMEM;
	TrkIv *hv = c->p_tiv.as<TrkIv>();
	memcpy(hv, iv.data(), niv * sizeof(TrkIv));
	{ TrkIv &u = hv[niv]; memset(&u, 0, sizeof(u)); u.wbase = n_items; u.chr = -1; }
	const i64 nbin = c->track_nwin;
	const i64 nwg_c = (items + 255) / 256, nwg_e = (n_items + 255) / 256;
	ENS(TrkBlk, d_tblk, (size_t)nt + 1); ENS(TrkIv, d_tiv, niv + 1); ENS(i64, d_twg, (size_t)nwg_e + 2);      // sums | {records without a job, columns outside their record}
	// the dense array: allocated and cleared once -- a call that grew it, or one that failed between COUNT and EMIT, clears it again
	{
		const size_t had = c->d_tbin.cap;
		ENS(uint4, d_tbin, (size_t)nbin);
		if (c->d_tbin.cap != had) c->track_zeroed = 0;
		if (c->track_dirty || c->track_zeroed < (size_t)nbin) {
			GSA_CHECK(c, hipMemsetAsync(c->d_tbin.p, 0, (size_t)nbin * sizeof(uint4), st));
			c->track_zeroed = (size_t)nbin; c->track_dirty = false;
		}
	}
	i64 *wg = c->d_twg.as<i64>(); unsigned long long *bad = (unsigned long long *)(wg + nwg_e);
	i64 *hdr = c->p_thdr.as<i64>();
	GSA_CHECK(c, hipMemcpyAsync(c->d_tblk.p, c->p_tblk.p, ((size_t)nt + 1) * sizeof(TrkBlk), hipMemcpyHostToDevice, st));
	GSA_CHECK(c, hipMemcpyAsync(c->d_tiv.p, hv, (niv + 1) * sizeof(TrkIv), hipMemcpyHostToDevice, st));
	GSA_CHECK(c, hipMemsetAsync(bad, 0, 2 * sizeof(unsigned long long), st));
	TrkIn a;
	gap_in_fill(c, a);
	a.blk = c->d_tblk.as<TrkBlk>(); a.nb = nt; a.n = items; a.iv = c->d_tiv.as<TrkIv>(); a.niv = (i32)niv; a.n_items = n_items;
	a.W = W; a.nbin = nbin; a.bin = c->d_tbin.as<u32>(); a.n_out = 0;
	c->track_dirty = true;      // (until EMIT has run)
	hipLaunchKernelGGL(k_trk_count, dim3((unsigned)nwg_c), dim3(256), 0, st, a, bad);
	GSA_CHECK(c, hipGetLastError());
	hipLaunchKernelGGL(k_trk_own, dim3((unsigned)nwg_e), dim3(256), 0, st, a, wg);
	GSA_CHECK(c, hipGetLastError());
	hipLaunchKernelGGL(k_trk_scan, dim3(1), dim3(256), 0, st, nwg_e, wg, (const unsigned long long *)bad, hdr);
	GSA_CHECK(c, hipGetLastError());
	GSA_CHECK(c, hipStreamSynchronize(st));
	const i64 nw = hdr[0];
	if (hdr[1]) return gsa_fail(c, GSA_ERR_STATE, "internal: gsa_ref_track met " + std::to_string((long long)hdr[1]) + " DP record(s) without a DP job");
	if (hdr[2]) return gsa_fail(c, GSA_ERR_STATE, "internal: gsa_ref_track met " + std::to_string((long long)hdr[2]) + " column(s) outside the record or sequence that should hold them");
	if (nw <= 0 || nw > n_items) return gsa_fail(c, GSA_ERR_STATE, "internal: gsa_ref_track counted more windows than the intervals touch");
	// the output is sized from the scan's total; it goes home in one copy
	ENS(gsa_track_win, d_tout, (size_t)nw); if (!pin_ensure<gsa_track_win>(c, c->p_tout, (size_t)nw)) return GSA_ERR_NOMEM;
	a.n_out = nw;
	hipLaunchKernelGGL(k_trk_emit, dim3((unsigned)nwg_e), dim3(256), 0, st, a, (const i64 *)wg, c->d_tout.as<gsa_track_win>());
	GSA_CHECK(c, hipGetLastError());
	GSA_CHECK(c, hipMemcpyAsync(c->p_tout.p, c->d_tout.p, (size_t)nw * sizeof(gsa_track_win), hipMemcpyDeviceToHost, st));
	GSA_CHECK(c, hipStreamSynchronize(st));
	c->track_dirty = false;
	out->n_win = nw; out->win = c->p_tout.as<gsa_track_win>();
	return GSA_OK;
}
