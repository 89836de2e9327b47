// gsalign_amd/csrc/k_lift.hip -- gsa_lift: reference positions carried through a stage-8 result to the query contig (include/gsa_hip.h), on the
// device, over what stage 8 left there.
//
// One position per lane.  A position p of the forward reference is text position p for forward-strand blocks and 2G - 1 - p for reverse-strand blocks; the blocks of
// both strands stand in ONE table sorted by their first text position, with the running maximum of their (clamped) ends beside it, so for either text position t the
// covering blocks are found by a search for the last block that starts at or before t and a scan backwards while the running maximum still lies above t.
//   COVER   per position: the covering blocks counted, the best one chosen (not a duplicate, then score, then index) -> pick[]; hits per workgroup -> wg[]
//   SCAN    one workgroup turns the workgroups' sums into their first slots; the host reads the total and sizes the output
//   EMIT    per position with a block: the record of the block that holds t (the last one with rpos <= t), then the column -- a seed answers at once, a gap of at
//           most LIFT_SERIAL columns is walked by its lane, a longer one by a wavefront in 64-column steps; the hit goes to its slot, so hits are dense and ascending
// No workgroup waits for another, nothing spins.  As in the other passes the columns of a DP gap come from the op string of its DP job (gsa_walk.h), never from the
// string pools.
#include <algorithm>
#include <cstring>
#include "gsa_fm.h"
#include "gsa_walk.h"

#define LIFT_SERIAL 64      // gap records of at most this many columns are walked by one lane, longer ones by a wavefront in 64-column steps

// one block with records, in the order of `start`: the text positions it covers [start, end) (end clamped to its chromosome copy), the greatest end of the entries up to
// this one, its records (absolute), and what the choice and the hit need
struct LiftBlk { i64 start, end, maxend, frag_off; i32 n_frag, score, bdup, block, rev, _pad; };
struct LiftPick { i32 ent; uint16_t n_cover, _pad; };      // the chosen table entry (-1: no block covers the position)
struct LiftIn : GapIn {
	const LiftBlk *blk; i32 nb;
	const i64 *pos; i64 n, G;
	i32 qoff;                                                  // start of the contig in a bundle's concatenation
	i64 n_out;
};

__device__ __forceinline__ bool lift_better(const LiftBlk &x, const LiftBlk &y)
{
	if ((x.bdup != 0) != (y.bdup != 0)) return x.bdup == 0;
	if (x.score != y.score) return x.score > y.score;
	return x.block < y.block;
}

// the blocks that cover text position t: counted into n, the best of them (and of `best`) into best
__device__ __forceinline__ void lift_cover(const LiftIn &a, i64 t, i32 &best, u32 &n)
{
	if (a.blk[0].start > t) return;
	for (i32 j = blk_last_le(a.blk, a.nb, &LiftBlk::start, t); j >= 0 && a.blk[j].maxend > t; j--) {
		if (a.blk[j].end <= t) continue;
		n++;
		if (best < 0 || lift_better(a.blk[j], a.blk[best])) best = j;
	}
}

__global__ void __launch_bounds__(256) k_lift_cover(LiftIn a, LiftPick *pick, i64 *wg)
{
	__shared__ i32 s_w[4];
	const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
	const i64 w = (i64)blockIdx.x * 256 + tid;
	i32 best = -1; u32 n = 0;
	if (w < a.n) {
		const i64 p = a.pos[w];
		lift_cover(a, p, best, n);
		lift_cover(a, 2 * a.G - 1 - p, best, n);
		LiftPick k; k.ent = best; k.n_cover = (uint16_t)(n > 65535u ? 65535u : n); k._pad = 0;
		pick[w] = k;
	}
	i32 tot = best >= 0 ? 1 : 0;
	for (int d = 32; d; d >>= 1) tot += __shfl_xor(tot, d);
	if (lane == 0) s_w[wv] = tot;
	__syncthreads();
	if (tid == 0) wg[blockIdx.x] = (i64)s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

__global__ void __launch_bounds__(256) k_lift_scan(i64 nwg, i64 *wg, i64 *hdr)
{
	__shared__ i64 s_w[4];
	const i64 total = wg_scan_sums(wg, nwg, s_w);
	if (threadIdx.x == 0) hdr[0] = total;
}

// what EMIT knows of a position before it looks at a column
struct LiftAt { i64 i = 0, t = 0; gsa_frag f; i32 ftype = 0; gsa_lift_hit h; };

__device__ __forceinline__ LiftAt lift_at(const LiftIn &a, i64 w, const LiftPick &pk)
{
	LiftAt x;
	const LiftBlk b = a.blk[pk.ent];
	const i64 p = a.pos[w];
	x.t = b.rev ? 2 * a.G - 1 - p : p;
	i64 lo = b.frag_off, hi = b.frag_off + b.n_frag;      // (the block's first record starts at b.start <= t)
	while (hi - lo > 1) { const i64 m = (lo + hi) >> 1; if (a.frag[m].rpos <= x.t) lo = m; else hi = m; }
	x.i = lo; x.f = a.frag[lo]; x.ftype = a.ftype[lo];
	x.h.idx = (int32_t)w; x.h.qpos = -1; x.h.block = b.block; x.h.cls = 0; x.h.rev = (uint8_t)b.rev; x.h.n_cover = pk.n_cover;
	return x;
}

__device__ __forceinline__ uint8_t lift_pair(uint8_t r, uint8_t q) { const int x = gsa_nt4(r); return (uint8_t)((x < 4 && x == gsa_nt4(q)) ? GSA_CIGAR_EQ : GSA_CIGAR_X); }

__device__ __forceinline__ void lift_put(const LiftIn &a, gsa_lift_hit *out, i64 slot, gsa_lift_hit h, i32 qp, uint8_t cls)
{
	h.qpos = qp - a.qoff; h.cls = cls;
	if (slot >= 0 && slot < a.n_out) out[slot] = h;
}

// the column of reference base t inside a gap of at most LIFT_SERIAL columns (op[0 .. L)), by one lane; false: the ops do not reach it
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
		if (ch != 'D') rp++;
		if (ch != 'I') qp++;
	}
	return false;
}

// the same by a whole wavefront, 64 columns per step: a lane's reference / query position is the step's base plus the number of lower lanes whose column consumes a
// base of that side; the lane whose column consumes reference base t answers
__device__ bool lift_wave(const LiftIn &a, const LiftAt &x, const uint8_t *op, i32 L, gsa_lift_hit *out, i64 slot)
{
	const int lane = threadIdx.x & 63;
	const unsigned long long below = (1ull << lane) - 1ull;
	i64 rp0 = x.f.rpos; i32 qp0 = x.f.qpos;
	for (i32 base = 0; base < L; base += 64) {
		const i32 p = base + lane;
		const int ch = p < L ? (int)op[p] : 0;
		const bool c1 = ch == 'M' || ch == 'I', c2 = ch == 'M' || ch == 'D';
		const unsigned long long m1 = __ballot(c1), m2 = __ballot(c2);
		const i64 rp = rp0 + __popcll(m1 & below); const i32 qp = qp0 + __popcll(m2 & below);
		const bool me = c1 && rp == x.t && (ch == 'I' || qp - x.f.qpos < x.f.qlen);
		if (me) { if (ch == 'I') lift_put(a, out, slot, x.h, qp - 1, (uint8_t)GSA_CIGAR_DEL); else lift_put(a, out, slot, x.h, qp, lift_pair(a.ref[rp], a.query[qp])); }
		if (__ballot(me)) return true;
		rp0 += __popcll(m1); qp0 += __popcll(m2);
		if (rp0 > x.t) return false;
	}
	return false;
}

// bad[0]: DP records without a DP job, bad[1]: positions their record (or its ops) does not hold -- neither can happen; both are counted and reported, never skipped silently
__global__ void __launch_bounds__(256) k_lift_emit(LiftIn a, const LiftPick *pick, const i64 *wg, unsigned long long *bad, gsa_lift_hit *out)
{
	__shared__ i32 s_list[256], s_w[4];
	__shared__ i64 s_slot[256];
	__shared__ int s_n;
	const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
	const i64 w = (i64)blockIdx.x * 256 + tid;
	if (tid == 0) s_n = 0;
	LiftPick pk; pk.ent = -1; pk.n_cover = 0; pk._pad = 0;
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
		else if (L > LIFT_SERIAL) { const int at = atomicAdd(&s_n, 1); s_list[at] = tid; s_slot[tid] = slot; }
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
	if (!pin_ensure<LiftBlk>(c, c->p_lblk, nb) || !pin_ensure<i64>(c, c->p_lhdr, 4)) return GSA_ERR_NOMEM;
	// the block table: a few KB from the blocks and their first and last records, which the host holds
	LiftBlk *hb = c->p_lblk.as<LiftBlk>(); i32 nt = 0;
	const gsa_rec *recs = c->p_frags.as<gsa_rec>() + rr.f0;
	for (size_t j = 0; j < nb; j++) {
		const gsa_block &bl = c->h_blocks[rr.b0 + j];
		if (bl.n_frag <= 0) continue;
		gsa_frag first, last;
		gsa_rec_expand(recs, bl.frag_off, &first); gsa_rec_expand(recs, bl.frag_off + bl.n_frag - 1, &last);
		const i64 fwd = c->h_chr_fwd[(size_t)bl.chr], len = c->h_chr_len[(size_t)bl.chr];
		const i64 lim = bl.bdir ? fwd + len : 2 * c->G - fwd;      // end of the block's chromosome copy (iExtension, tools.cpp:192-202)
		LiftBlk &v = hb[nt];
		v.start = first.rpos; v.end = std::min<i64>(last.rpos + last.rlen, lim); v.maxend = 0;
		v.frag_off = bl.frag_off + rr.f0; v.n_frag = bl.n_frag; v.score = bl.score; v.bdup = bl.bdup; v.block = (i32)j; v.rev = bl.bdir ? 0 : 1; v._pad = 0;
		if (v.end > v.start) nt++;
	}
	if (nt == 0) return GSA_OK;
	std::sort(hb, hb + nt, [](const LiftBlk &x, const LiftBlk &y) { return x.start != y.start ? x.start < y.start : x.block < y.block; });
	for (i32 j = 0; j < nt; j++) hb[j].maxend = j ? std::max(hb[j - 1].maxend, hb[j].end) : hb[j].end;
	const i64 nwg = (n + 255) / 256;
	ENS(LiftBlk, d_lblk, (size_t)nt); ENS(LiftPick, d_lpick, (size_t)n); ENS(i64, d_lwg, (size_t)nwg + 2);      // sums | {records without a job, positions outside their record}
	i64 *wg = c->d_lwg.as<i64>(); unsigned long long *bad = (unsigned long long *)(wg + nwg);
	i64 *hdr = c->p_lhdr.as<i64>();
	GSA_CHECK(c, hipMemcpyAsync(c->d_lblk.p, hb, (size_t)nt * sizeof(LiftBlk), hipMemcpyHostToDevice, st));
	GSA_CHECK(c, hipMemsetAsync(bad, 0, 2 * sizeof(unsigned long long), st));
	LiftIn a;
	gap_in_fill(c, a);
	a.blk = c->d_lblk.as<LiftBlk>(); a.nb = nt; a.pos = c->d_lpos.as<i64>(); a.n = n; a.G = c->G; a.qoff = rr.qoff; a.n_out = 0;
	hipLaunchKernelGGL(k_lift_cover, dim3((unsigned)nwg), dim3(256), 0, st, a, c->d_lpick.as<LiftPick>(), wg);
	GSA_CHECK(c, hipGetLastError());
	hipLaunchKernelGGL(k_lift_scan, dim3(1), dim3(256), 0, st, nwg, wg, hdr);
	GSA_CHECK(c, hipGetLastError());
	GSA_CHECK(c, hipStreamSynchronize(st));
	const i64 nh = hdr[0];
	if (nh < 0 || nh > n) return gsa_fail(c, GSA_ERR_STATE, "internal: gsa_lift counted more hits than positions");
	if (nh == 0) return GSA_OK;
	// the output is sized from the scan's total; it goes home in one copy
	ENS(gsa_lift_hit, d_lhit, (size_t)nh); if (!pin_ensure<gsa_lift_hit>(c, c->p_lhit, (size_t)nh)) return GSA_ERR_NOMEM;
	a.n_out = nh;
	hipLaunchKernelGGL(k_lift_emit, dim3((unsigned)nwg), dim3(256), 0, st, a, (const LiftPick *)c->d_lpick.as<LiftPick>(), (const i64 *)wg, bad, c->d_lhit.as<gsa_lift_hit>());
	GSA_CHECK(c, hipGetLastError());
	GSA_CHECK(c, hipMemcpyAsync(c->p_lhit.p, c->d_lhit.p, (size_t)nh * sizeof(gsa_lift_hit), hipMemcpyDeviceToHost, st));
	GSA_CHECK(c, hipMemcpyAsync(hdr + 1, bad, 2 * sizeof(i64), hipMemcpyDeviceToHost, st));
	GSA_CHECK(c, hipStreamSynchronize(st));
	if (hdr[1]) return gsa_fail(c, GSA_ERR_STATE, "internal: gsa_lift met " + std::to_string((long long)hdr[1]) + " DP record(s) without a DP job");
	if (hdr[2]) return gsa_fail(c, GSA_ERR_STATE, "internal: gsa_lift met " + std::to_string((long long)hdr[2]) + " position(s) outside the record that should hold them");
	out->n_hits = nh; out->hits = c->p_lhit.as<gsa_lift_hit>();
	return GSA_OK;
}
