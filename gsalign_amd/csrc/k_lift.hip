// gsalign_amd/csrc/k_lift.hip -- gsa_lift: reference positions carried through a stage-8 result to the query contig (include/gsa_hip.h), on the
// device, over what stage 8 left there.
//
// One position per lane.  A position p of the forward reference is text position p for forward-strand blocks and 2G - 1 - p for reverse-strand blocks; the blocks of
// both strands stand in ONE table sorted by their first text position, with the running maximum of their (clamped) ends beside it (gsa_walk.h's span table, which
// k_regions.hip reads too), so for either text position t the covering blocks are found by the cover search of the one-base interval [t, t + 1).
//   COVER   per position: the covering blocks counted, the best one chosen (not a duplicate, then score, then index) -> pick[]; hits per workgroup -> wg[]
//   SCAN    one workgroup turns the workgroups' sums into their first slots; the host reads the total and sizes the output
//   EMIT    per position with a block: the record of the block that holds t (the last one with rpos <= t), then the column -- a seed answers at once, a gap of at
//           most WALK_SERIAL columns is walked by its lane, a longer one by a wavefront in 64-column steps; the hit goes to its slot, so hits are dense and ascending
// No workgroup waits for another, nothing spins.  As in the other passes the columns of a DP gap come from the op string of its DP job (gsa_walk.h), never from the
// string pools.
#include "gsa_walk.h"

struct LiftIn : GapIn {
	const SpanBlk *blk; i32 nb;
	const i64 *pos; i64 n, G;
	i32 qoff;                                                  // start of the contig in a bundle's concatenation
	i64 n_out;
};

// (the overlaps of a one-base interval are all 1: the choice is score, then index)
__global__ void __launch_bounds__(256) k_lift_cover(LiftIn a, SpanPick *pick, i64 *wg)
{
	__shared__ i32 s_w[4];
	const i64 w = (i64)blockIdx.x * 256 + threadIdx.x;
	SpanPick k; k.ent = -1;
	if (w < a.n) { const i64 p = a.pos[w]; pick[w] = k = span_pick(a.blk, a.nb, a.G, p, p + 1); }
	wg_count(k.ent >= 0, s_w, wg);
}

// what EMIT knows of a position before it looks at a column
struct LiftAt { i64 i = 0, t = 0; gsa_frag f; i32 ftype = 0; gsa_lift_hit h; };

__device__ __forceinline__ LiftAt lift_at(const LiftIn &a, i64 w, const SpanPick &pk)
{
	LiftAt x;
	const SpanBlk b = a.blk[pk.ent];
	const i64 p = a.pos[w];
	x.t = b.rev ? 2 * a.G - 1 - p : p;
	x.i = span_rec_of(a.frag, b.frag_off, b.frag_off + b.n_frag, x.t);      // (the block's first record starts at b.start <= t)
	x.f = a.frag[x.i]; x.ftype = a.ftype[x.i];
	x.h.idx = (int32_t)w; x.h.qpos = -1; x.h.block = b.block; x.h.cls = 0; x.h.rev = (uint8_t)b.rev; x.h.n_cover = pk.n_cover;
	return x;
}

__device__ __forceinline__ uint8_t lift_pair(uint8_t r, uint8_t q) { return (uint8_t)(col_mismatch(r, q) ? GSA_CIGAR_X : GSA_CIGAR_EQ); }

__device__ __forceinline__ void lift_put(const LiftIn &a, gsa_lift_hit *out, i64 slot, gsa_lift_hit h, i32 qp, uint8_t cls)
{
	h.qpos = qp - a.qoff; h.cls = cls;
	if (slot >= 0 && slot < a.n_out) out[slot] = h;
}

// the column of reference base t inside a gap of at most WALK_SERIAL columns (op[0 .. L)), by one lane; false: the ops do not reach it
__device__ bool lift_lane(const LiftIn &a, const LiftAt &x, const uint8_t *op, i32 L, gsa_lift_hit *out, i64 slot)
{
	i64 rp = x.f.rpos; i32 qp = x.f.qpos;
	for (i32 i = 0; i < L; i++) {
		const int ch = (int)op[i];
		if (ch != 'D' && rp == x.t) {
			if (ch == 'I') { lift_put(a, out, slot, x.h, qp - 1, (uint8_t)GSA_CIGAR_DEL); return true; }
			if (qp - x.f.qpos >= x.f.qlen) return false;
			lift_put(a, out, slot, x.h, qp, lift_pair(a.ref[rp], a.query[qp]));
			return true;
		}
		col_advance(ch, rp, qp);
	}
	return false;
}

// the same by a whole wavefront, 64 columns per step (wave_step): the lane whose column consumes reference base t answers
__device__ bool lift_wave(const LiftIn &a, const LiftAt &x, const uint8_t *op, i32 L, gsa_lift_hit *out, i64 slot)
{
	i64 rp0 = x.f.rpos; i32 qp0 = x.f.qpos;
	for (i32 base = 0; base < L; base += 64) {
		const WaveCol w = wave_step(op, L, base, rp0, qp0);
		const bool me = w.c1 && w.rp == x.t && (w.ch == 'I' || w.qp - x.f.qpos < x.f.qlen);
		if (me) { if (w.ch == 'I') lift_put(a, out, slot, x.h, w.qp - 1, (uint8_t)GSA_CIGAR_DEL); else lift_put(a, out, slot, x.h, w.qp, lift_pair(a.ref[w.rp], a.query[w.qp])); }
		if (__ballot(me)) return true;
		if (rp0 > x.t) return false;
	}
	return false;
}

// bad[0]: DP records without a DP job, bad[1]: positions their record (or its ops) does not hold -- neither can happen; both are counted and reported, never skipped silently
__global__ void __launch_bounds__(256) k_lift_emit(LiftIn a, const SpanPick *pick, const i64 *wg, unsigned long long *bad, gsa_lift_hit *out)
{
	__shared__ i32 s_list[256], s_w[4];
	__shared__ i64 s_slot[256];
	__shared__ int s_n;
	const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
	const i64 w = (i64)blockIdx.x * 256 + tid;
	if (tid == 0) s_n = 0;
	SpanPick pk; pk.ent = -1; pk.n_cover = 0; pk._pad = 0;
	if (w < a.n) pk = pick[w];
	const bool hit = pk.ent >= 0;
	const i64 slot = wg[blockIdx.x] + wg_excl_scan<i32>(hit ? 1 : 0, s_w);      // (its barrier also publishes s_n = 0)
	if (hit) {
		const LiftAt x = lift_at(a, w, pk);
		const i64 d = x.t - x.f.rpos;
		const uint8_t *op = nullptr; i32 L = 0;
		if (d < 0 || d >= (i64)x.f.rlen) { atomicAdd(bad + 1, 1ull); lift_put(a, out, slot, x.h, a.qoff - 1, 0); }
		else if (x.ftype == FT_SEED) lift_put(a, out, slot, x.h, x.f.qpos + (i32)d, (uint8_t)GSA_CIGAR_EQ);
		else if (x.f.qlen <= 0) lift_put(a, out, slot, x.h, x.f.qpos - 1, (uint8_t)GSA_CIGAR_DEL);      // (a pure deletion: the base in front of it is the last base of the seed in front)
		else if (!gap_ops(a, x.i, x.ftype, x.f, op, L)) { atomicAdd(bad, 1ull); lift_put(a, out, slot, x.h, a.qoff - 1, 0); }
		else if (!op) {                                      // (an equal-length gap that needed no DP: L = qlen columns of 'M')
			if (d < (i64)L) lift_put(a, out, slot, x.h, x.f.qpos + (i32)d, lift_pair(a.ref[x.t], a.query[x.f.qpos + d]));
			else { atomicAdd(bad + 1, 1ull); lift_put(a, out, slot, x.h, a.qoff - 1, 0); }
		}
		else if (L > WALK_SERIAL) { const int at = atomicAdd(&s_n, 1); s_list[at] = tid; s_slot[tid] = slot; }
		else if (!lift_lane(a, x, op, L, out, slot)) { atomicAdd(bad + 1, 1ull); lift_put(a, out, slot, x.h, a.qoff - 1, 0); }
	}
	__syncthreads();
	const int nlist = s_n;
	for (int q = wv; q < nlist; q += 4) {
		// (the position's look-up is repeated by every lane of the wavefront: the addresses are uniform, so the loads are one request each)
		const int t = s_list[q];
		const i64 wt = (i64)blockIdx.x * 256 + t;
		const LiftAt x = lift_at(a, wt, pick[wt]);
		const uint8_t *op = nullptr; i32 L = 0;
		const bool ok = gap_ops(a, x.i, x.ftype, x.f, op, L) && op && lift_wave(a, x, op, L, out, s_slot[t]);
		if (!ok && lane == 0) { atomicAdd(bad + 1, 1ull); lift_put(a, out, s_slot[t], x.h, a.qoff - 1, 0); }
	}
}

int lift_positions(gsa_ctx *c, i32 k, gsa_lifts *out)
{
	const ResultRange rr = result_range(c, k);
	const size_t nb = rr.nb;
	const i64 n = c->lift_n;
	if (nb == 0 || c->n_frags <= 0 || n <= 0) return GSA_OK;
	if (!c->result_pinned) return gsa_fail(c, GSA_ERR_STATE, "gsa_lift: the context holds no finished (stage 8) result");
	hipStream_t st = c->stream;
	if (!pin_ensure<i64>(c, c->p_lhdr, 4)) return GSA_ERR_NOMEM;
	i32 nt = 0; i64 W = 0;      // (every block with records, sorted)
	if (const int rc = span_build<SpanBlk>(c, rr, "gsa_lift", c->p_lblk, SPAN_SORT, span_keep_all, span_no_extra, nt, W)) return rc;
	if (nt == 0) return GSA_OK;
	const i64 nwg = (n + 255) / 256;
	ENS(SpanBlk, d_lblk, (size_t)nt); ENS(SpanPick, d_lpick, (size_t)n); ENS(i64, d_lwg, (size_t)nwg + 2);      // sums | {records without a job, positions outside their record}
	i64 *wg = c->d_lwg.as<i64>(); unsigned long long *bad = (unsigned long long *)(wg + nwg);
	i64 *hdr = c->p_lhdr.as<i64>();
	GSA_CHECK(c, hipMemcpyAsync(c->d_lblk.p, c->p_lblk.p, (size_t)nt * sizeof(SpanBlk), hipMemcpyHostToDevice, st));
	GSA_CHECK(c, hipMemsetAsync(bad, 0, 2 * sizeof(unsigned long long), st));
	LiftIn a;
	gap_in_fill(c, a);
	a.blk = c->d_lblk.as<SpanBlk>(); a.nb = nt; a.pos = c->d_lpos.as<i64>(); a.n = n; a.G = c->G; a.qoff = rr.qoff; a.n_out = 0;
	hipLaunchKernelGGL(k_lift_cover, dim3((unsigned)nwg), dim3(256), 0, st, a, c->d_lpick.as<SpanPick>(), wg);
	GSA_CHECK(c, hipGetLastError());
	hipLaunchKernelGGL(k_wg_total<>, dim3(1), dim3(256), 0, st, nwg, wg, hdr);
	GSA_CHECK(c, hipGetLastError());
	GSA_CHECK(c, hipStreamSynchronize(st));
	const i64 nh = hdr[0];
	if (nh < 0 || nh > n) return gsa_fail(c, GSA_ERR_STATE, "internal: gsa_lift counted more hits than positions");
	if (nh == 0) return GSA_OK;
	// the output is sized from the scan's total; it goes home in one copy
	ENS(gsa_lift_hit, d_lhit, (size_t)nh); if (!pin_ensure<gsa_lift_hit>(c, c->p_lhit, (size_t)nh)) return GSA_ERR_NOMEM;
	a.n_out = nh;
	hipLaunchKernelGGL(k_lift_emit, dim3((unsigned)nwg), dim3(256), 0, st, a, (const SpanPick *)c->d_lpick.as<SpanPick>(), (const i64 *)wg, bad, c->d_lhit.as<gsa_lift_hit>());
	GSA_CHECK(c, hipGetLastError());
	GSA_CHECK(c, hipMemcpyAsync(c->p_lhit.p, c->d_lhit.p, (size_t)nh * sizeof(gsa_lift_hit), hipMemcpyDeviceToHost, st));
	GSA_CHECK(c, hipMemcpyAsync(hdr + 1, bad, 2 * sizeof(i64), hipMemcpyDeviceToHost, st));
	GSA_CHECK(c, hipStreamSynchronize(st));
	if (hdr[1]) return gsa_fail(c, GSA_ERR_STATE, "internal: gsa_lift met " + std::to_string((long long)hdr[1]) + " DP record(s) without a DP job");
	if (hdr[2]) return gsa_fail(c, GSA_ERR_STATE, "internal: gsa_lift met " + std::to_string((long long)hdr[2]) + " position(s) outside the record that should hold them");
	out->n_hits = nh; out->hits = c->p_lhit.as<gsa_lift_hit>();
	return GSA_OK;
}
