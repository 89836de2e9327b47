// gsalign_amd/csrc/k_regions.hip -- gsa_lift_regions: reference intervals carried through a stage-8 result to the query contig (include/gsa_hip.h), on
// the device, over what stage 8 left there.
//
// A region [beg, end) of the forward reference is the text interval [beg, end) for forward-strand blocks and [2G - end, 2G - beg) for reverse-strand blocks.  The blocks
// of both strands stand in gsa_walk.h's span table, the one k_lift.hip reads (sorted by first text position, running maximum of the clamped ends beside it, every
// block's first work item), so the same table serves the cover search and the per-record passes.  The two end columns of a region are two walks; everything between them is a difference of a
// per-record prefix, so no column of the records in between is looked at.
//   CLASS   one work item per record of the table's blocks: the record's four counts {eq, x, del, ins}, untrimmed, for the whole record.  A seed, a pure deletion and
//           a pure insertion are arithmetic; a gap of at most WALK_SERIAL columns is walked by its lane, a longer one goes through s_list / s_n to a wavefront that takes
//           64 columns per step with ballot / popcount.  The same launch leaves the exclusive prefix inside the workgroup and the workgroups' sums
//   SCAN    one workgroup turns the four arrays of sums into the workgroups' first values;  ADD makes the prefix global.  (uint32_t, modulo 2^32 from end to end: only
//           differences inside ONE block are ever taken, and those are below 2^31.)  CLASS, SCAN and ADD depend on the result only, not on the regions
//   COVER   one region per lane: for each of its two text intervals a search for the last block that starts below t_hi and a scan backwards while the running maximum
//           lies above t_lo; the overlapping blocks counted, the best one chosen (not a duplicate, then overlap, then score, then index) -> pick[]; hits per workgroup -> wg[]
//   SCAN    the workgroups' sums into their first slots; the host reads the total and sizes the output
//   EMIT    per region with a block: the records that hold t_lo and t_hi - 1 (two searches), the prefix difference of the records strictly between them, and the
//           partial counts of the two end records -- arithmetic for run records, a walk for gaps, by lane or by wavefront under the same rule.  Both ends in ONE record:
//           that record is walked once, from the first column of the span to the last.  The hit goes to its slot, so hits are dense and ascending
// Neighbouring lanes of COVER and EMIT handle neighbouring regions: sorted input gives near-uniform search addresses; nothing depends on the order.  No workgroup waits
// for another, nothing spins.  As in the other passes the columns of a DP gap come from the op string of its DP job (gsa_walk.h), never from the string pools.
#include "gsa_walk.h"

struct RegIn : GapIn {
	const SpanBlk *blk; i32 nb;
	i64 W;                                                     // records of the table's blocks: the work items of CLASS, the entries of pre
	const uint4 *pre;                                          // per record: {eq, x, del, ins} of the records in front of it (EMIT)
	const i64 *beg, *end; i64 n, G;
	i32 qoff, qtot;                                            // start of the contig in a bundle's concatenation; bases the device copy holds
	i64 n_out;
};
// bad[0]: DP records without a DP job, bad[1]: spans their records (or their ops) do not reach -- neither can happen; both are counted and reported, never skipped silently
enum { RG_NOJOB = 0, RG_OUT = 1 };

// counts of a stretch of columns and the query position in front of its first column
struct RegPart { u32 eq = 0, x = 0, del = 0, ins = 0; i32 q = 0; };
__device__ __forceinline__ void reg_sum(RegPart &t, const RegPart &r) { t.eq += r.eq; t.x += r.x; t.del += r.del; t.ins += r.ins; }

// The columns of a gap (op[0 .. L), null: 'M' throughout) from the column that holds reference base ta (clip_lo; else from the first column) through the column that
// holds tb (clip_hi; else through the last), by one lane.  'D' puts '-' into the reference row (CIGAR I), 'I' into the query row (CIGAR D).  false: the ops do not
// reach the span, or leave the record
__device__ bool reg_lane(const RegIn &a, const gsa_frag &f, const uint8_t *op, i32 L, bool clip_lo, i64 ta, bool clip_hi, i64 tb, RegPart &r)
{
	i64 rp = f.rpos; i32 qp = f.qpos; bool in = !clip_lo, done = false;
	r.q = f.qpos;
	for (i32 i = 0; i < L && !done; i++) {
		const int ch = op ? (int)op[i] : (int)'M';
		if ((ch != 'D' && (rp - f.rpos >= f.rlen || rp >= 2 * a.G)) || (ch != 'I' && (qp - f.qpos >= f.qlen || qp < 0 || qp >= a.qtot))) return false;
		if (!in && ch != 'D' && rp == ta) { in = true; r.q = qp; }
		if (in) {
			if (ch == 'D') r.ins++;
			else if (ch == 'I') r.del++;
			else if (col_mismatch(a.ref[rp], a.query[qp])) r.x++;
			else r.eq++;
			if (clip_hi && ch != 'D' && rp == tb) done = true;
		}
		col_advance(ch, rp, qp);
	}
	return in && (done || (!clip_hi && rp - f.rpos == f.rlen && qp - f.qpos == f.qlen));
}

// the same by a whole wavefront, 64 columns per step (wave_step): the lanes between the span's first and last column count, every lane ends with the same r
__device__ bool reg_wave(const RegIn &a, const gsa_frag &f, const uint8_t *op, i32 L, bool clip_lo, i64 ta, bool clip_hi, i64 tb, RegPart &r)
{
	const int lane = threadIdx.x & 63;
	i64 rp0 = f.rpos; i32 qp0 = f.qpos; bool in = !clip_lo, done = false;
	r.q = f.qpos;
	for (i32 base = 0; base < L && !done; base += 64) {
		const WaveCol w = wave_step(op, L, base, rp0, qp0);
		const int ch = w.ch; const bool c1 = w.c1, c2 = w.c2; const i64 rp = w.rp; const i32 qp = w.qp;
		const bool out = (c1 && (rp - f.rpos >= f.rlen || rp >= 2 * a.G)) || (c2 && (qp - f.qpos >= f.qlen || qp < 0 || qp >= a.qtot));
		if (__ballot(out)) return false;
		unsigned long long span = ~0ull;                   // the step's lanes inside the span
		if (!in) {
			const unsigned long long ms = __ballot(c1 && rp == ta);
			if (ms) { const int s = __ffsll((long long)ms) - 1; in = true; r.q = __shfl(qp, s); span = ~0ull << s; }
			else span = 0ull;
		}
		if (in && clip_hi) {
			const unsigned long long me = __ballot(c1 && rp == tb);
			if (me) { const int e = __ffsll((long long)me) - 1; done = true; if (e < 63) span &= (1ull << (e + 1)) - 1ull; }
		}
		const bool mine = ch != 0 && ((span >> lane) & 1ull);
		const bool mm = mine && ch == 'M' && col_mismatch(a.ref[rp], a.query[qp]);
		r.eq += (u32)__popcll(__ballot(mine && ch == 'M' && !mm)); r.x += (u32)__popcll(__ballot(mm));
		r.del += (u32)__popcll(__ballot(mine && ch == 'I')); r.ins += (u32)__popcll(__ballot(mine && ch == 'D'));
	}
	return in && (done || (!clip_hi && rp0 - f.rpos == f.rlen && qp0 - f.qpos == f.qlen));
}

// What a stretch of record i costs: RG_DONE r holds the answer (a run record: arithmetic), RG_WALK op[0 .. L) has to be walked, RG_BADJOB a DP record without a DP
// job, RG_BADSPAN the record does not hold the span.  ta / tb as in reg_lane
enum { RG_DONE = 0, RG_WALK = 1, RG_BADJOB = 2, RG_BADSPAN = 3, RG_QUEUED = 4 };
__device__ __forceinline__ int reg_piece(const RegIn &a, i64 i, const gsa_frag &f, i32 ftype, bool clip_lo, i64 ta, bool clip_hi, i64 tb, RegPart &r, const uint8_t *&op, i32 &L)
{
	const i64 d0 = clip_lo ? ta - f.rpos : 0, d1 = clip_hi ? tb - f.rpos : (i64)f.rlen - 1;
	if ((clip_lo || clip_hi) && (d0 < 0 || d1 < d0 || d1 >= (i64)f.rlen)) return RG_BADSPAN;
	r.q = f.qpos;
	if (ftype == FT_SEED) { if (f.rlen > 0) { r.eq = (u32)(d1 - d0 + 1); r.q = f.qpos + (i32)d0; } return RG_DONE; }
	if (f.rlen <= 0) { if (f.qlen > 0) r.ins = (u32)f.qlen; return RG_DONE; }      // (a pure insertion; it holds no reference base, so it is never clipped)
	if (f.qlen <= 0) { r.del = (u32)(d1 - d0 + 1); return RG_DONE; }                // (a pure deletion: the next query base is the one behind it)
	if (!gap_ops(a, i, ftype, f, op, L)) return RG_BADJOB;
	return L > 0 ? RG_WALK : RG_BADSPAN;
}

// the record of CLASS work item w
struct RegRec { i64 i; gsa_frag f; i32 ftype; };
__device__ __forceinline__ RegRec reg_rec(const RegIn &a, i64 w)
{
	RegRec x;
	const SpanBlk b = a.blk[blk_last_le(a.blk, a.nb, &SpanBlk::wbase, w)];
	x.i = b.frag_off + (w - b.wbase);
	x.f = a.frag[x.i]; x.ftype = a.ftype[x.i];
	return x;
}

// wg: four arrays of nwg sums {eq | x | del | ins}
__global__ void __launch_bounds__(256) k_reg_class(RegIn a, uint4 *pre, i64 *wg, i64 nwg, unsigned long long *bad)
{
	__shared__ i32 s_list[256];
	__shared__ u32 s_v[256][4], s_w[16];
	__shared__ int s_n;
	const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
	const i64 w = (i64)blockIdx.x * 256 + tid;
	if (tid == 0) s_n = 0;
	__syncthreads();
	u32 v[4] = { 0, 0, 0, 0 };
	bool queued = false;
	if (w < a.W) {
		const RegRec x = reg_rec(a, w);
		RegPart r; const uint8_t *op = nullptr; i32 L = 0;
		int kind = reg_piece(a, x.i, x.f, x.ftype, false, 0, false, 0, r, op, L);
		if (kind == RG_WALK) {
			if (L > WALK_SERIAL) { s_list[atomicAdd(&s_n, 1)] = tid; queued = true; kind = RG_QUEUED; }
			else if (!reg_lane(a, x.f, op, L, false, 0, false, 0, r)) kind = RG_BADSPAN;
		}
		if (kind == RG_BADJOB) atomicAdd(bad + RG_NOJOB, 1ull);
		else if (kind == RG_BADSPAN) atomicAdd(bad + RG_OUT, 1ull);
		else if (kind != RG_QUEUED) { v[0] = r.eq; v[1] = r.x; v[2] = r.del; v[3] = r.ins; }
	}
	__syncthreads();
	const int nlist = s_n;
	for (int q = wv; q < nlist; q += 4) {
		// (the record's look-up is repeated by every lane of the wavefront: the addresses are uniform, so the loads are one request each)
		const int t = s_list[q];
		const RegRec x = reg_rec(a, (i64)blockIdx.x * 256 + t);
		RegPart r; const uint8_t *op = nullptr; i32 L = 0;
		const bool ok = reg_piece(a, x.i, x.f, x.ftype, false, 0, false, 0, r, op, L) == RG_WALK && reg_wave(a, x.f, op, L, false, 0, false, 0, r);
		if (lane == 0) {
			if (!ok) { atomicAdd(bad + RG_OUT, 1ull); r = RegPart(); }
			s_v[t][0] = r.eq; s_v[t][1] = r.x; s_v[t][2] = r.del; s_v[t][3] = r.ins;
		}
	}
	__syncthreads();
	if (queued) { v[0] = s_v[tid][0]; v[1] = s_v[tid][1]; v[2] = s_v[tid][2]; v[3] = s_v[tid][3]; }
	const u32 own[4] = { v[0], v[1], v[2], v[3] };
	wg_excl_scan<u32, 4>(v, s_w);
	if (w < a.W) pre[w] = make_uint4(v[0], v[1], v[2], v[3]);
	if (tid == 255)
#pragma unroll
		for (int k = 0; k < 4; k++) wg[(i64)k * nwg + blockIdx.x] = (i64)(u32)(v[k] + own[k]);
}

__global__ void __launch_bounds__(256) k_reg_class_scan(i64 nwg, i64 *wg)
{
	__shared__ i64 s_w[4];
	for (int k = 0; k < 4; k++) { wg_scan_sums(wg + (i64)k * nwg, nwg, s_w); __syncthreads(); }
}

__global__ void __launch_bounds__(256) k_reg_class_add(i64 W, uint4 *pre, const i64 *wg, i64 nwg)
{
	const i64 w = (i64)blockIdx.x * 256 + threadIdx.x;
	if (w >= W) return;
	uint4 p = pre[w];
	p.x += (u32)wg[blockIdx.x]; p.y += (u32)wg[nwg + blockIdx.x]; p.z += (u32)wg[2 * nwg + blockIdx.x]; p.w += (u32)wg[3 * nwg + blockIdx.x];
	pre[w] = p;
}

// the choice: not a duplicate, then the greater overlap, then the greater score, then the smaller block index (span_better)
__global__ void __launch_bounds__(256) k_reg_cover(RegIn a, SpanPick *pick, i64 *wg)
{
	__shared__ i32 s_w[4];
	const i64 w = (i64)blockIdx.x * 256 + threadIdx.x;
	SpanPick k; k.ent = -1;
	if (w < a.n) pick[w] = k = span_pick(a.blk, a.nb, a.G, a.beg[w], a.end[w]);
	wg_count(k.ent >= 0, s_w, wg);
}

// what EMIT knows of a region before it looks at a column: the span [t_lo, t_hi), the records iA / iB that hold t_lo / t_hi - 1, the hit without its counts
struct RegAt { SpanBlk b; i64 t_lo = 0, t_hi = 0, iA = 0, iB = 0; gsa_region_hit h; };

__device__ __forceinline__ RegAt reg_at(const RegIn &a, i64 w, const SpanPick &pk)
{
	RegAt x;
	x.b = a.blk[pk.ent];
	const i64 beg = a.beg[w], end = a.end[w];
	const i64 lo = x.b.rev ? 2 * a.G - end : beg, hi = x.b.rev ? 2 * a.G - beg : end;
	x.t_lo = lo > x.b.start ? lo : x.b.start; x.t_hi = hi < x.b.end ? hi : x.b.end;
	x.iA = span_rec_of(a.frag, x.b.frag_off, x.b.frag_off + x.b.n_frag, x.t_lo);
	x.iB = span_rec_of(a.frag, x.iA, x.b.frag_off + x.b.n_frag, x.t_hi - 1);
	memset(&x.h, 0, sizeof(x.h));
	x.h.idx = (int32_t)w; x.h.block = x.b.block; x.h.rev = (uint8_t)x.b.rev; x.h.n_cover = pk.n_cover;
	x.h.off_lo = (int32_t)(x.b.rev ? hi - x.t_hi : x.t_lo - lo); x.h.off_hi = (int32_t)(x.b.rev ? hi - x.t_lo : x.t_hi - lo);
	return x;
}

// the stretch of end record `which` (0: the record of t_lo, clipped in front -- and behind when it holds t_hi - 1 too; 1: the record of t_hi - 1, clipped behind)
__device__ __forceinline__ int reg_end_piece(const RegIn &a, const RegAt &x, int which, gsa_frag &f, bool &clip_lo, bool &clip_hi, RegPart &r, const uint8_t *&op, i32 &L)
{
	const i64 i = which ? x.iB : x.iA;
	f = a.frag[i];
	clip_lo = which == 0; clip_hi = which == 1 || x.iA == x.iB;
	return reg_piece(a, i, f, a.ftype[i], clip_lo, x.t_lo, clip_hi, x.t_hi - 1, r, op, L);
}

__global__ void __launch_bounds__(256) k_reg_emit(RegIn a, const SpanPick *pick, const i64 *wg, unsigned long long *bad, gsa_region_hit *out)
{
	__shared__ i32 s_list[512], s_w[4], s_q[256];
	__shared__ u32 s_v[256][4];
	__shared__ int s_n;
	const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
	const i64 w = (i64)blockIdx.x * 256 + tid;
	if (tid == 0) s_n = 0;
	s_v[tid][0] = s_v[tid][1] = s_v[tid][2] = s_v[tid][3] = 0u; s_q[tid] = 0;
	SpanPick pk; pk.ent = -1; pk.n_cover = 0; pk._pad = 0;
	if (w < a.n) pk = pick[w];
	const bool hit = pk.ent >= 0 && pk.ent < a.nb;
	const i64 slot = wg[blockIdx.x] + wg_excl_scan<i32>(hit ? 1 : 0, s_w);      // (its barrier also publishes s_n = 0 and the cleared rows)
	RegAt x; RegPart tot; bool q0 = false, q1 = false, fail = false;
	if (hit) {
		x = reg_at(a, w, pk);
		if (x.t_hi <= x.t_lo) fail = true;
		for (int which = 0; which < 2 && !fail; which++) {
			if (which == 1 && x.iB == x.iA) break;
			gsa_frag f; bool cl, ch; RegPart r; const uint8_t *op = nullptr; i32 L = 0;
			int kind = reg_end_piece(a, x, which, f, cl, ch, r, op, L);
			if (kind == RG_WALK) {
				if (L > WALK_SERIAL) { s_list[atomicAdd(&s_n, 1)] = 2 * tid + which; if (which) q1 = true; else q0 = true; kind = RG_QUEUED; }
				else if (!reg_lane(a, f, op, L, cl, x.t_lo, ch, x.t_hi - 1, r)) kind = RG_BADSPAN;
			}
			if (kind == RG_BADJOB) { atomicAdd(bad + RG_NOJOB, 1ull); fail = true; }
			else if (kind == RG_BADSPAN) { atomicAdd(bad + RG_OUT, 1ull); fail = true; }
			else if (kind != RG_QUEUED) { reg_sum(tot, r); if (which == 0) tot.q = r.q; }
		}
		if (!fail && x.iB > x.iA + 1) {          // the records strictly between the two ends: a difference of the prefix, no column is looked at
			const i64 wa = x.b.wbase + (x.iA + 1 - x.b.frag_off), wb = x.b.wbase + (x.iB - x.b.frag_off);
			if (wa < 0 || wb >= a.W) { atomicAdd(bad + RG_OUT, 1ull); fail = true; }
			else { const uint4 pa = a.pre[wa], pb = a.pre[wb]; tot.eq += pb.x - pa.x; tot.x += pb.y - pa.y; tot.del += pb.z - pa.z; tot.ins += pb.w - pa.w; }
		}
	}
	__syncthreads();
	const int nlist = s_n;
	for (int q = wv; q < nlist; q += 4) {
		// (the region's look-up is repeated by every lane of the wavefront: the addresses are uniform, so the loads are one request each)
		const int t = s_list[q] >> 1, which = s_list[q] & 1;
		const i64 wt = (i64)blockIdx.x * 256 + t;
		const RegAt y = reg_at(a, wt, pick[wt]);
		gsa_frag f; bool cl, ch; RegPart r; const uint8_t *op = nullptr; i32 L = 0;
		const bool ok = reg_end_piece(a, y, which, f, cl, ch, r, op, L) == RG_WALK && reg_wave(a, f, op, L, cl, y.t_lo, ch, y.t_hi - 1, r);
		if (lane == 0) {
			if (!ok) atomicAdd(bad + RG_OUT, 1ull);
			else {      // (a region's two ends may be walked by two wavefronts at once)
				atomicAdd(&s_v[t][0], r.eq); atomicAdd(&s_v[t][1], r.x); atomicAdd(&s_v[t][2], r.del); atomicAdd(&s_v[t][3], r.ins);
				if (which == 0) s_q[t] = r.q;
			}
		}
	}
	__syncthreads();
	if (!hit) return;
	if (q0 || q1) { tot.eq += s_v[tid][0]; tot.x += s_v[tid][1]; tot.del += s_v[tid][2]; tot.ins += s_v[tid][3]; }
	if (q0) tot.q = s_q[tid];
	gsa_region_hit h = x.h;
	if (fail) { h.q_lo = h.q_hi = -1; }
	else {
		// (every column counted in eq / x / del holds one reference base of the span: a sum that differs means the records did not reach it)
		if ((i64)tot.eq + tot.x + tot.del != x.t_hi - x.t_lo) atomicAdd(bad + RG_OUT, 1ull);
		h.q_lo = tot.q - a.qoff; h.q_hi = h.q_lo + (int32_t)(tot.eq + tot.x + tot.ins);
		h.n_eq = tot.eq; h.n_x = tot.x; h.n_del = tot.del; h.n_ins = tot.ins;
	}
	if (slot >= 0 && slot < a.n_out) out[slot] = h;
}

int lift_regions(gsa_ctx *c, i32 k, gsa_region_lifts *out)
{
	const ResultRange rr = result_range(c, k);
	const size_t nb = rr.nb;
	const i64 n = c->reg_n;
	if (nb == 0 || c->n_frags <= 0 || n <= 0) return GSA_OK;
	if (!c->result_pinned) return gsa_fail(c, GSA_ERR_STATE, "gsa_lift_regions: the context holds no finished (stage 8) result");
	hipStream_t st = c->stream;
	if (!pin_ensure<i64>(c, c->p_rghdr, 4)) return GSA_ERR_NOMEM;
	// lift_positions' table, in its buffers: each call builds it and has consumed it before it returns
	i32 nt = 0; i64 W = 0;
	if (const int rc = span_build<SpanBlk>(c, rr, "gsa_lift_regions", c->p_lblk, SPAN_SORT, span_keep_all, span_no_extra, nt, W)) return rc;
	if (nt == 0) return GSA_OK;
	const i64 nwg = (n + 255) / 256, nwg_c = (W + 255) / 256;
	ENS(SpanBlk, d_lblk, (size_t)nt); ENS(SpanPick, d_lpick, (size_t)n); ENS(uint4, d_rgpre, (size_t)W);
	ENS(i64, d_rgwg, (size_t)nwg + 2 + 4 * (size_t)nwg_c);      // the regions' sums | {records without a job, spans outside their records} | the records' four arrays of sums
	i64 *wg = c->d_rgwg.as<i64>(); unsigned long long *bad = (unsigned long long *)(wg + nwg); i64 *wg_c = wg + nwg + 2;
	i64 *hdr = c->p_rghdr.as<i64>();
	GSA_CHECK(c, hipMemcpyAsync(c->d_lblk.p, c->p_lblk.p, (size_t)nt * sizeof(SpanBlk), hipMemcpyHostToDevice, st));
	GSA_CHECK(c, hipMemsetAsync(bad, 0, 2 * sizeof(unsigned long long), st));
	RegIn a;
	gap_in_fill(c, a);
	a.blk = c->d_lblk.as<SpanBlk>(); a.nb = nt; a.W = W; a.pre = c->d_rgpre.as<uint4>();
	a.beg = c->d_rgpos.as<i64>(); a.end = a.beg + n; a.n = n; a.G = c->G;
	a.qoff = rr.qoff; a.qtot = c->bnd.n ? c->b_off[(size_t)c->bnd.n] : c->qlen; a.n_out = 0;
	// CLASS + PREFIX: of the result alone
	hipLaunchKernelGGL(k_reg_class, dim3((unsigned)nwg_c), dim3(256), 0, st, a, c->d_rgpre.as<uint4>(), wg_c, nwg_c, bad);
	GSA_CHECK(c, hipGetLastError());
	hipLaunchKernelGGL(k_reg_class_scan, dim3(1), dim3(256), 0, st, nwg_c, wg_c);
	GSA_CHECK(c, hipGetLastError());
	hipLaunchKernelGGL(k_reg_class_add, dim3((unsigned)nwg_c), dim3(256), 0, st, W, c->d_rgpre.as<uint4>(), (const i64 *)wg_c, nwg_c);
	GSA_CHECK(c, hipGetLastError());
	hipLaunchKernelGGL(k_reg_cover, dim3((unsigned)nwg), dim3(256), 0, st, a, c->d_lpick.as<SpanPick>(), wg);
	GSA_CHECK(c, hipGetLastError());
	hipLaunchKernelGGL(k_wg_total<>, dim3(1), dim3(256), 0, st, nwg, wg, hdr);
	GSA_CHECK(c, hipGetLastError());
	GSA_CHECK(c, hipStreamSynchronize(st));
	const i64 nh = hdr[0];
	if (nh < 0 || nh > n) return gsa_fail(c, GSA_ERR_STATE, "internal: gsa_lift_regions counted more hits than regions");
	if (nh > 0) {
		// the output is sized from the scan's total; it goes home in one copy
		ENS(gsa_region_hit, d_rghit, (size_t)nh); if (!pin_ensure<gsa_region_hit>(c, c->p_rghit, (size_t)nh)) return GSA_ERR_NOMEM;
		a.n_out = nh;
		hipLaunchKernelGGL(k_reg_emit, dim3((unsigned)nwg), dim3(256), 0, st, a, (const SpanPick *)c->d_lpick.as<SpanPick>(), (const i64 *)wg, bad, c->d_rghit.as<gsa_region_hit>());
		GSA_CHECK(c, hipGetLastError());
		GSA_CHECK(c, hipMemcpyAsync(c->p_rghit.p, c->d_rghit.p, (size_t)nh * sizeof(gsa_region_hit), hipMemcpyDeviceToHost, st));
	}
	GSA_CHECK(c, hipMemcpyAsync(hdr + 1, bad, 2 * sizeof(i64), hipMemcpyDeviceToHost, st));
	GSA_CHECK(c, hipStreamSynchronize(st));
	if (hdr[1]) return gsa_fail(c, GSA_ERR_STATE, "internal: gsa_lift_regions met " + std::to_string((long long)hdr[1]) + " DP record(s) without a DP job");
	if (hdr[2]) return gsa_fail(c, GSA_ERR_STATE, "internal: gsa_lift_regions met " + std::to_string((long long)hdr[2]) + " span(s) the records that should hold them do not reach");
	if (nh == 0) return GSA_OK;
	out->n_hits = nh; out->hits = c->p_rghit.as<gsa_region_hit>();
	return GSA_OK;
}
