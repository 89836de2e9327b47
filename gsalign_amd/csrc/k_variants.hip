// gsalign_amd/csrc/k_variants.hip -- gsa_call_variants: VariantIdentification (reference src/SeqVariant.cpp:12-119) on the
// device, over what stage 8 left there.
//
// A variant is a local event of one non-seed record: where it starts is a predicate on a column and the column before it,
// its reference / query position is the record's plus the number of earlier columns that are not '-' on that side.  So:
// a COUNT pass (variants per record), an exclusive scan (two levels: per workgroup, then one workgroup over the
// workgroups' sums), and an EMIT pass that repeats the walk and stores every variant at its slot -- the serial order of
// the reference (blocks in result order, records in order, columns in order) without any serial step, no workgroup
// waits for another.
//
// The columns of a record are not read from the string pools: the strings of the large DP jobs were written straight
// into pinned host memory (k_materialize_large) and never existed in d_tail.  They are DERIVED, for every walked record
// alike, from what is on the device for all of them: the forward M/D/I op string of its DP job (d_ops, or e_ops for the
// jobs launched early) and the two sequences -- an aligned column is the sequence byte or '-' (ksw2_alignment.cpp:264-272:
// 'D' puts '-' into aln1, 'I' into aln2); an equal-length gap that needed no DP is all 'M'.  One byte per column instead
// of two, and one code path.
#include "gsa_walk.h"

struct VarBlk { i64 frag_off; i32 n_frag, chr, block, wbase; };      // one surviving, non-duplicate block: first record (absolute), records, its reference sequence, index in gsa_result::blocks, first work item
struct VarIn : GapIn {
	i32 nvb; i64 W; const VarBlk *blk;
	i32 qoff;                                                          // start of the contig in a bundle's concatenation
	const i64 *chr_end; i32 n_ends; i64 G;
	i64 n_out;
};

enum { VC_NONE = 0, VC_DEL = 1, VC_INS = 2, VC_ONE = 3, VC_WALK = 4 };
struct VarGap { i32 cls = VC_NONE, L = 0; const uint8_t *op = nullptr; i32 qpos = 0, qlen = 0, rlen = 0; i64 rpos = 0; };
enum { VC_BAD = 5 };      // a DP record without a DP job (gap_ops): counted and reported

__device__ __forceinline__ VarGap var_load(const VarIn &a, i64 i)
{
	VarGap g;
	const i32 t = a.ftype[i];
	if (t == FT_SEED) return g;
	const gsa_frag f = a.frag[i];
	g.qpos = f.qpos; g.qlen = f.qlen; g.rlen = f.rlen; g.rpos = f.rpos;
	if (f.qlen == 0 && f.rlen == 0) return g;                       // (:31)
	if (f.qlen == 0) g.cls = VC_DEL;
	else if (f.rlen == 0) g.cls = VC_INS;
	else if (f.qlen == 1 && f.rlen == 1) g.cls = VC_ONE;
	else g.cls = gap_ops(a, i, t, f, g.op, g.L) ? VC_WALK : VC_BAD;
	return g;
}

// GenCoordinateInfo(p).gPos (tools.cpp:120-140; HostIndex::coordinate): the position's own look-up in ChrLocMap
__device__ __forceinline__ i32 var_pos(const VarIn &a, i64 p)
{
	i32 lo = 0, hi = a.n_ends;
	while (lo < hi) { const i32 m = (lo + hi) >> 1; if (a.chr_end[m] < p) lo = m + 1; else hi = m; }
	if (lo >= a.n_ends) lo = a.n_ends - 1;
	if (p < a.G) return (i32)(p + 1 - (lo ? a.chr_end[lo - 1] + 1 : 0));
	return (i32)(a.chr_end[lo] - p + 1);
}

__device__ __forceinline__ void var_put(const VarIn &a, gsa_variant *out, i64 slot, const VarBlk &vb, i32 kind, i64 rpos, i32 qpos, i32 len)
{
	if (slot < 0 || slot >= a.n_out) return;
	gsa_variant v; v.rpos = rpos; v.qpos = qpos - a.qoff; v.len = len; v.chr = vb.chr; v.pos = var_pos(a, rpos); v.kind = kind; v.block = vb.block;
	out[slot] = v;
}

// substitution test of one aligned column (:54, :97-99)
__device__ __forceinline__ bool var_subst(uint8_t a1, uint8_t a2) { const int x = gsa_nt4(a2); return x != 4 && x != gsa_nt4(a1); }

// everything but a long walk, by one lane; returns the number of variants, kinds into cnt[] (substitutions, insertions, deletions)
template <bool EMIT>
__device__ i32 var_lane(const VarIn &a, const VarGap &g, const VarBlk &vb, gsa_variant *out, i64 slot, i32 cnt[3])
{
	if (g.cls == VC_DEL) { cnt[2]++; if (EMIT) var_put(a, out, slot, vb, 2, g.rpos - 1, g.qpos - 1, g.rlen); return 1; }      // (:32-41)
	if (g.cls == VC_INS) { cnt[1]++; if (EMIT) var_put(a, out, slot, vb, 1, g.rpos - 1, g.qpos - 1, g.qlen); return 1; }      // (:42-51)
	if (g.cls == VC_ONE) {                                                                                                       // (:52-63)
		if (!var_subst(a.ref[g.rpos], a.query[g.qpos])) return 0;
		cnt[0]++; if (EMIT) var_put(a, out, slot, vb, 0, g.rpos, g.qpos, 0);
		return 1;
	}
	i64 rp = g.rpos; i32 qp = g.qpos, n = 0;                                                                                     // (:64-115)
	for (i32 i = 0; i < g.L; i++) {
		const uint8_t ch = g.op ? g.op[i] : (uint8_t)'M';
		if (ch == 'D' || ch == 'I') {
			i32 run = 1; while (i + run < g.L && g.op[i + run] == ch) run++;
			if (ch == 'D') { cnt[1]++; if (EMIT) var_put(a, out, slot + n, vb, 3, rp - 1, qp - 1, run); qp += run; }           // aln1 has '-': insertion
			else { cnt[2]++; if (EMIT) var_put(a, out, slot + n, vb, 4, rp - 1, qp - 1, run); rp += run; }                     // aln2 has '-': deletion
			n++; i += run - 1;
		} else {
			if (var_subst(a.ref[rp], a.query[qp])) { cnt[0]++; if (EMIT) var_put(a, out, slot + n, vb, 0, rp, qp, 0); n++; }
			rp++; qp++;
		}
	}
	return n;
}

// a long walk by a whole wavefront, 64 columns per step (wave_step): a lane's slot is the step's base plus the number of lower lanes that start a variant
template <bool EMIT>
__device__ i32 var_wave(const VarIn &a, const VarGap &g, const VarBlk &vb, gsa_variant *out, i64 slot, i32 cnt[3])
{
	const int lane = threadIdx.x & 63;
	const unsigned long long below = (1ull << lane) - 1ull;
	i64 rp0 = g.rpos; i32 qp0 = g.qpos, n = 0; int carry = 0;      // carry: the column in front of the step
	for (i32 base = 0; base < g.L; base += 64) {
		const WaveCol w = wave_step(g.op, g.L, base, rp0, qp0);
		const i32 p = w.p; const int ch = w.ch; const i64 rp = w.rp; const i32 qp = w.qp;
		int pch = __shfl_up(ch, 1); if (lane == 0) pch = carry;
		const bool ins = ch == 'D' && pch != 'D', del = ch == 'I' && pch != 'I';
		const bool sub = ch == 'M' && var_subst(a.ref[rp], a.query[qp]);
		const bool st = ins || del || sub;
		const unsigned long long ms = __ballot(st);
		cnt[0] += sub; cnt[1] += ins; cnt[2] += del;
		if (EMIT && st) {
			i32 run = 0;
			if (!sub) { run = 1; while (p + run < g.L && g.op[p + run] == ch) run++; }
			var_put(a, out, slot + n + __popcll(ms & below), vb, sub ? 0 : (ins ? 3 : 4), sub ? rp : rp - 1, sub ? qp : qp - 1, run);
		}
		n += __popcll(ms); carry = __shfl(ch, 63);
	}
	return n;
}

// One work item per record of the listed blocks, a workgroup per 256 of them.  EMIT = false: variants per record -> nv[], per workgroup -> wg[], per kind -> kinds[];
// EMIT = true: wg[] holds the workgroups' first slots, a record's slot is that plus the exclusive sum of nv[] in front of it inside the workgroup.
template <bool EMIT>
__global__ void __launch_bounds__(256) k_var_pass(VarIn a, i32 *nv, i64 *wg, unsigned long long *kinds, gsa_variant *out)
{
	__shared__ i32 s_list[256], s_val[256], s_w[4], s_k[3];
	__shared__ int s_n;
	const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
	const i64 w = (i64)blockIdx.x * 256 + tid;
	if (tid == 0) s_n = 0;
	if (tid < 3) s_k[tid] = 0;
	VarGap g;
	i32 b = 0;
	if (w < a.W) {
		b = blk_last_le(a.blk, a.nvb, &VarBlk::wbase, w);
		g = var_load(a, a.blk[b].frag_off + (w - a.blk[b].wbase));
	}
	i32 cnt[3] = { 0, 0, 0 };
	i64 slot = 0;
	const i64 wgb = EMIT ? wg[blockIdx.x] : 0;      // the workgroup's first slot
	if (EMIT) slot = wgb + wg_excl_scan<i32>(w < a.W ? nv[w] : 0, s_w);      // the workgroup's first slot plus the counts in front of the record inside it
	__syncthreads();
	const bool wide = g.cls == VC_WALK && g.L > WALK_SERIAL;
	i32 n = 0;
	if (wide) { const int at = atomicAdd(&s_n, 1); s_list[at] = tid; }
	else if (g.cls == VC_BAD) { if (!EMIT) atomicAdd(&kinds[3], 1ull); }
	else if (g.cls != VC_NONE) n = var_lane<EMIT>(a, g, a.blk[b], out, slot, cnt);
	s_val[tid] = EMIT ? (i32)(slot - wgb) : 0;
	__syncthreads();
	const int nlist = s_n;
	for (int q = wv; q < nlist; q += 4) {
		// (the record's look-up is repeated by every lane of the wavefront: the addresses are uniform, so the loads are one request each)
		const int t = s_list[q];
		const i64 wt = (i64)blockIdx.x * 256 + t;
		const i32 lo = blk_last_le(a.blk, a.nvb, &VarBlk::wbase, wt);
		const VarGap gt = var_load(a, a.blk[lo].frag_off + (wt - a.blk[lo].wbase));
		const i32 nt = var_wave<EMIT>(a, gt, a.blk[lo], out, EMIT ? wgb + s_val[t] : 0, cnt);
		if (!EMIT && lane == 0) s_val[t] = nt;
	}
	if (EMIT) return;      // (safe: nothing below this line is reached on the EMIT path, so no __syncthreads is left waiting for these threads)
	__syncthreads();
	if (wide) n = s_val[tid];
	if (w < a.W) nv[w] = n;
	i32 tot = n;
	for (int d = 32; d; d >>= 1) { tot += __shfl_xor(tot, d); cnt[0] += __shfl_xor(cnt[0], d); cnt[1] += __shfl_xor(cnt[1], d); cnt[2] += __shfl_xor(cnt[2], d); }
	if (lane == 0) { s_w[wv] = tot; for (int k = 0; k < 3; k++) if (cnt[k]) atomicAdd(&s_k[k], cnt[k]); }
	__syncthreads();
	if (tid == 0) wg[blockIdx.x] = (i64)s_w[0] + s_w[1] + s_w[2] + s_w[3];
	if (tid < 3 && s_k[tid]) atomicAdd(&kinds[tid], (unsigned long long)s_k[tid]);
}

// second level of the scan: one workgroup turns the workgroups' sums into their first slots; total and kind counts go to the host's header
__global__ void __launch_bounds__(256) k_var_scan(i64 nwg, i64 *wg, const unsigned long long *kinds, i64 *hdr)
{
	__shared__ i64 s_w[4];
	const i64 total = wg_scan_sums(wg, nwg, s_w);
	if (threadIdx.x == 0) { hdr[0] = total; hdr[1] = (i64)kinds[0]; hdr[2] = (i64)kinds[1]; hdr[3] = (i64)kinds[2]; hdr[4] = (i64)kinds[3]; }
}

int call_variants(gsa_ctx *c, i32 k, gsa_variants *out)
{
	const ResultRange rr = result_range(c, k);
	const size_t nb = rr.nb;
	if (nb == 0 || c->n_frags <= 0) return GSA_OK;
	hipStream_t st = c->stream;
	if (!pin_ensure<VarBlk>(c, c->p_vblk, nb + 1) || !pin_ensure<i64>(c, c->p_vhdr, 5)) return GSA_ERR_NOMEM;
	VarBlk *hb = c->p_vblk.as<VarBlk>(); i32 nvb = 0; i64 W = 0;
	for (size_t j = 0; j < nb; j++) {
		const gsa_block &bl = c->h_blocks[rr.b0 + j];
		if (bl.bdup || bl.n_frag <= 0) continue;                    // (:22)
		VarBlk &v = hb[nvb++]; v.frag_off = bl.frag_off + rr.f0; v.n_frag = bl.n_frag; v.chr = bl.chr; v.block = (i32)j; v.wbase = (i32)W;
		W += bl.n_frag;
	}
	if (W == 0) return GSA_OK;
	if (W >= (1ll << 31) - 256) return gsa_fail(c, GSA_ERR_LIMIT, "gsa_call_variants: too many records");
	const bool timed = c->prof_var;      // (gsa_set_profiling bit 3: two events around the pass)
	if (timed && !c->ev_var[0]) { GSA_CHECK(c, hipEventCreate(&c->ev_var[0])); GSA_CHECK(c, hipEventCreate(&c->ev_var[1])); }
	const i64 nwg = (W + 255) / 256;
	ENS(VarBlk, d_vblk, (size_t)nvb + 1); ENS(i32, d_vcnt, (size_t)W + 1); ENS(i64, d_vwg, (size_t)nwg + 4);      // sums | {substitutions, insertions, deletions, records without a job}
	unsigned long long *kinds = (unsigned long long *)(c->d_vwg.as<i64>() + nwg);
	i64 *hdr = c->p_vhdr.as<i64>();
	GSA_CHECK(c, hipMemcpyAsync(c->d_vblk.p, hb, (size_t)nvb * sizeof(VarBlk), hipMemcpyHostToDevice, st));
	if (timed) GSA_CHECK(c, hipEventRecord(c->ev_var[0], st));
	GSA_CHECK(c, hipMemsetAsync(kinds, 0, 4 * sizeof(unsigned long long), st));
	VarIn a;
	a.nvb = nvb; a.W = W; a.blk = c->d_vblk.as<VarBlk>();
	gap_in_fill(c, a); a.qoff = rr.qoff;
	a.chr_end = c->di.chr_end; a.n_ends = c->di.n_ends; a.G = c->di.G; a.n_out = 0;
	hipLaunchKernelGGL(k_var_pass<false>, dim3((unsigned)nwg), dim3(256), 0, st, a, c->d_vcnt.as<i32>(), c->d_vwg.as<i64>(), kinds, (gsa_variant *)nullptr);
	hipLaunchKernelGGL(k_var_scan, dim3(1), dim3(256), 0, st, nwg, c->d_vwg.as<i64>(), (const unsigned long long *)kinds, hdr);
	GSA_CHECK(c, hipGetLastError());
	GSA_CHECK(c, hipStreamSynchronize(st));
	const i64 n = hdr[0];
	if (hdr[4]) return gsa_fail(c, GSA_ERR_STATE, "internal: gsa_call_variants met " + std::to_string((long long)hdr[4]) + " DP record(s) without a DP job");
	if (n > 0) {
		// the output is sized from the scan's total; it goes home in one copy
		ENS(gsa_variant, d_var, (size_t)n); if (!pin_ensure<gsa_variant>(c, c->p_var, (size_t)n)) return GSA_ERR_NOMEM;
		a.n_out = n;
		hipLaunchKernelGGL(k_var_pass<true>, dim3((unsigned)nwg), dim3(256), 0, st, a, c->d_vcnt.as<i32>(), c->d_vwg.as<i64>(), kinds, c->d_var.as<gsa_variant>());
		GSA_CHECK(c, hipGetLastError());
		GSA_CHECK(c, hipMemcpyAsync(c->p_var.p, c->d_var.p, (size_t)n * sizeof(gsa_variant), hipMemcpyDeviceToHost, st));
	}
	if (timed) GSA_CHECK(c, hipEventRecord(c->ev_var[1], st));
	GSA_CHECK(c, hipStreamSynchronize(st));
	if (timed) { float ms = 0; if (hipEventElapsedTime(&ms, c->ev_var[0], c->ev_var[1]) == hipSuccess) { c->pass_stat[PASS_VAR].ms_sum += ms; c->pass_stat[PASS_VAR].calls++; } (void)hipGetLastError(); }
	out->n = n; out->v = n ? c->p_var.as<gsa_variant>() : nullptr; out->n_snv = hdr[1]; out->n_ins = hdr[2]; out->n_del = hdr[3];
	return GSA_OK;
}
