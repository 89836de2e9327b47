// gsalign_amd/csrc/k_cigar.hip -- gsa_block_cigars: the CIGAR of every block of a stage-8 result (PAF's cg:Z:, include/gsa_hip.h), on the
// device, over what stage 8 left there.
//
// A block's CIGAR is the run-length encoding of its columns -- the columns of the two `s` lines OutputMAF prints (reference
// src/tools.cpp:165-216): a seed record is `len` columns of '=', a gap record the columns of its two gapped strings.  A run STARTS at a column
// whose class differs from the class of the column in front of it; for a record's first column that is the last column of the record in
// front of it in the same block ('=' behind a seed, the class of the last op behind a gap, nothing at the block's first record).  So a start
// is a local predicate, and runs merge across record boundaries by themselves.  One work item per record of the listed blocks:
//   COUNT   run starts and columns per record, per workgroup; columns per class per block (integer atomics: any order gives the same sums)
//   SCAN    one workgroup turns the workgroups' sums into their first slots / first columns, PREFIX gives every record its own
//   BLOCKS  a block's first op and op count are the prefix values at its first record and at the next block's
//   EMIT    the walk again: every start stores {column inside the block << 4 | class} at its slot
//   PACK    a run's length is the next start's column (or the block's column count) minus its own; op = len << 4 | class, stored at
//           slot k of the block -- at n_cig - 1 - k for a reverse-strand block: SelfComplementarySeq reverses the two lines, classes do
//           not change under complement, and merging is symmetric
// No workgroup waits for another, nothing spins.
// POS (block_cigars(.., pos = true), the front half of gsa_block_cs, k_cs.hip): the EMIT walk also stores, beside run[slot], the reference and query position of the
// run's first column in walk order, and counts the runs other than '=' that go on into the next record at a position that does not continue them.
//
// As in k_variants.hip the columns of a gap are DERIVED from the forward M/D/I op string of its DP job (d_ops, or e_ops for the jobs launched
// early) and the two sequences, never read from the string pools: the strings of the large DP jobs never exist in d_tail.  'D' puts '-' into
// the reference row (CIGAR I), 'I' into the query row (CIGAR D) (ksw2_alignment.cpp:264-272); an equal-length gap that needed no DP is all
// 'M'; a pure insertion / deletion record is one run whatever its length.
#include "gsa_walk.h"

struct CigIn : GapIn {
	i32 nb; i64 W; const CigBlk *blk;
	i64 n_out;
	i64 *run_r; i32 *run_q;                                           // POS only: position of every run's first column (walk order)
};

enum { CG_NONE = 0, CG_RUN = 1, CG_WALK = 2, CG_BAD = 3 };      // no column; L columns of one class; walked column by column; a DP record without a DP job (reported, never skipped)
struct CigRec { i32 kind = CG_NONE, L = 0, cls = 0; const uint8_t *op = nullptr; i32 qpos = 0, qlen = 0, rlen = 0; i64 rpos = 0; };

__device__ __forceinline__ CigRec cig_load(const CigIn &a, i64 i)
{
	CigRec g;
	const i32 t = a.ftype[i];
	const gsa_frag f = a.frag[i];
	g.qpos = f.qpos; g.qlen = f.qlen; g.rlen = f.rlen; g.rpos = f.rpos;
	if (t == FT_SEED) { if (f.qlen > 0) { g.kind = CG_RUN; g.L = f.qlen; g.cls = (i32)GSA_CIGAR_EQ; } return g; }
	if (f.qlen <= 0 && f.rlen <= 0) return g;
	if (f.qlen <= 0) { g.kind = CG_RUN; g.L = f.rlen; g.cls = (i32)GSA_CIGAR_DEL; return g; }
	if (f.rlen <= 0) { g.kind = CG_RUN; g.L = f.qlen; g.cls = (i32)GSA_CIGAR_INS; return g; }
	if (!gap_ops(a, i, t, f, g.op, g.L)) g.kind = CG_BAD;
	else if (g.L > 0) g.kind = CG_WALK;
	return g;
}

// class of a column that holds a base in both rows
__device__ __forceinline__ i32 cig_pair(uint8_t r, uint8_t q) { return col_mismatch(r, q) ? (i32)GSA_CIGAR_X : (i32)GSA_CIGAR_EQ; }
__device__ __forceinline__ i32 cig_class(const CigIn &a, int ch, i64 rp, i32 qp)
{
	return ch == 'D' ? (i32)GSA_CIGAR_INS : (ch == 'I' ? (i32)GSA_CIGAR_DEL : cig_pair(a.ref[rp], a.query[qp]));
}
__device__ __forceinline__ int cig_slot(i32 cls) { return cls == (i32)GSA_CIGAR_EQ ? 0 : (cls == (i32)GSA_CIGAR_X ? 1 : (cls == (i32)GSA_CIGAR_INS ? 2 : 3)); }      // order of gsa_block_cigar's counts

// class of the column in front of record i's first column: the last column of the nearest earlier record of the block that has one (records are
// seed [gap] seed ...: one or two steps); 0 at the block's first column
__device__ i32 cig_prev(const CigIn &a, const CigBlk &b, i64 i)
{
	for (i64 j = i - 1; j >= b.frag_off; j--) {
		const CigRec g = cig_load(a, j);
		if (g.kind == CG_RUN) return g.cls;
		if (g.kind == CG_BAD) return (i32)GSA_CIGAR_EQ;              // (the call fails)
		if (g.kind == CG_WALK) {
			const int ch = g.op ? (int)g.op[g.L - 1] : (int)'M';
			return cig_class(a, ch, g.rpos + g.rlen - 1, g.qpos + g.qlen - 1);      // (a last 'M' pairs the last base of either side)
		}
	}
	return 0;
}

template <bool POS>
__device__ __forceinline__ void cig_put(const CigIn &a, i64 *run, i64 slot, i64 col, i32 cls, i64 rp, i32 qp)
{
	if (slot >= 0 && slot < a.n_out) { run[slot] = (col << 4) | (i64)cls; if (POS) { a.run_r[slot] = rp; a.run_q[slot] = qp; } }
}

// POS: record i goes on with the run (class cls, not '=') the record in front of it ended with: 1 when the bases that run prints do not go on at (rpos, qpos)
__device__ i32 cig_gap_in_run(const CigIn &a, const CigBlk &b, i64 i, i32 cls, i64 rpos, i32 qpos)
{
	for (i64 j = i - 1; j >= b.frag_off; j--) {
		const CigRec g = cig_load(a, j);
		if (g.kind == CG_NONE) continue;
		if (g.kind == CG_BAD) return 0;
		const bool r_ok = cls == (i32)GSA_CIGAR_INS || g.rpos + (g.rlen > 0 ? g.rlen : 0) == rpos;      // (an insertion prints no reference base)
		const bool q_ok = cls == (i32)GSA_CIGAR_DEL || g.qpos + (g.qlen > 0 ? g.qlen : 0) == qpos;
		return (r_ok && q_ok) ? 0 : 1;
	}
	return 0;
}

// a run record or a short walk, by one lane; returns the number of run starts; columns per class into cnt[]
template <bool EMIT, bool POS>
__device__ i32 cig_lane(const CigIn &a, const CigRec &g, i32 prev, i64 *run, i64 slot, i64 col, i32 cnt[4])
{
	if (g.kind == CG_RUN) {
		cnt[cig_slot(g.cls)] += g.L;
		if (g.cls == prev) return 0;
		if (EMIT) cig_put<POS>(a, run, slot, col, g.cls, g.rpos, g.qpos);
		return 1;
	}
	i64 rp = g.rpos; i32 qp = g.qpos, n = 0;
	for (i32 i = 0; i < g.L; i++) {
		const int ch = g.op ? (int)g.op[i] : (int)'M';
		const i32 cls = cig_class(a, ch, rp, qp);
		cnt[cig_slot(cls)]++;
		if (cls != prev) { if (EMIT) cig_put<POS>(a, run, slot + n, col + i, cls, rp, qp); n++; prev = cls; }
		col_advance(ch, rp, qp);
	}
	return n;
}

// a long walk by a whole wavefront, 64 columns per step (wave_step): a lane's slot is the step's base plus the number of lower lanes that start a run
template <bool EMIT, bool POS>
__device__ i32 cig_wave(const CigIn &a, const CigRec &g, i32 prev, i64 *run, i64 slot, i64 col, i32 cnt[4])
{
	const int lane = threadIdx.x & 63;
	const unsigned long long below = (1ull << lane) - 1ull;
	i64 rp0 = g.rpos; i32 qp0 = g.qpos, n = 0; i32 carry = prev;      // carry: class of the column in front of the step
	for (i32 base = 0; base < g.L; base += 64) {
		const WaveCol w = wave_step(g.op, g.L, base, rp0, qp0);
		const bool valid = w.ch != 0;
		i32 cls = 0;
		if (valid) cls = w.ch == 'M' ? cig_pair(a.ref[w.rp], a.query[w.qp]) : (w.ch == 'D' ? (i32)GSA_CIGAR_INS : (i32)GSA_CIGAR_DEL);
		i32 pcls = __shfl_up(cls, 1); if (lane == 0) pcls = carry;
		const bool st = valid && cls != pcls;
		const unsigned long long ms = __ballot(st);
		if (valid) cnt[cig_slot(cls)]++;
		if (EMIT && st) cig_put<POS>(a, run, slot + n + __popcll(ms & below), col + w.p, cls, w.rp, w.qp);
		n += __popcll(ms); carry = __shfl(cls, 63);
	}
	return n;
}

// columns per class of one wavefront's records into their blocks' totals: one atomic per class when all its records lie in one block (the usual case)
__device__ __forceinline__ void cig_totals(gsa_block_cigar *out, bool active, i32 b, i32 cnt[4])
{
	const unsigned long long am = __ballot(active);
	if (!am) return;
	const i32 b0 = __shfl(b, __ffsll((long long)am) - 1);
	if (__ballot(active && b != b0) == 0ull) {
		i32 s[4];
		for (int k = 0; k < 4; k++) { s[k] = active ? cnt[k] : 0; for (int d = 32; d; d >>= 1) s[k] += __shfl_xor(s[k], d); }
		if ((threadIdx.x & 63) == 0) { if (s[0]) atomicAdd(&out[b0].n_eq, s[0]); if (s[1]) atomicAdd(&out[b0].n_x, s[1]); if (s[2]) atomicAdd(&out[b0].n_ins, s[2]); if (s[3]) atomicAdd(&out[b0].n_del, s[3]); }
	} else if (active) {
		if (cnt[0]) atomicAdd(&out[b].n_eq, cnt[0]); if (cnt[1]) atomicAdd(&out[b].n_x, cnt[1]); if (cnt[2]) atomicAdd(&out[b].n_ins, cnt[2]); if (cnt[3]) atomicAdd(&out[b].n_del, cnt[3]);
	}
}

// One work item per record of the listed blocks, a workgroup per 256 of them.  EMIT = false: run starts / columns per record -> ns[] / nc[], per workgroup -> wg[] / wg[nwg + ..],
// columns per class -> out[block]; EMIT = true: ps[] / pc[] hold every record's first slot and first column (global), the starts are stored into run[].
template <bool EMIT, bool POS>
__global__ void __launch_bounds__(256) k_cig_pass(CigIn a, i32 *ns, i32 *nc, i64 *wg, i64 nwg, unsigned long long *bad, gsa_block_cigar *out, const i64 *ps, const i64 *pc, i64 *run)
{
	__shared__ i32 s_list[256], s_val[256], s_prev[256];
	__shared__ i64 s_slot[256], s_col[256], s_w[8];
	__shared__ int s_n;
	const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
	const i64 w = (i64)blockIdx.x * 256 + tid;
	if (tid == 0) s_n = 0;
	CigRec g;
	i32 b = 0, prev = 0; i64 slot = 0, col = 0;
	const bool active = w < a.W;
	if (active) {
		b = blk_last_le(a.blk, a.nb, &CigBlk::wbase, w);      // (blocks without records share their wbase with the next one: the last of them is the one that has w)
		const i64 i = a.blk[b].frag_off + (w - a.blk[b].wbase);
		g = cig_load(a, i);
		if (g.kind == CG_RUN || g.kind == CG_WALK) prev = cig_prev(a, a.blk[b], i);
		if (EMIT) { slot = ps[w]; col = pc[w] - pc[a.blk[b].wbase]; }
		if (POS && prev != 0 && prev != (i32)GSA_CIGAR_EQ && (g.kind == CG_RUN || g.kind == CG_WALK)) {
			const i32 first = g.kind == CG_RUN ? g.cls : cig_class(a, g.op ? (int)g.op[0] : (int)'M', g.rpos, g.qpos);
			if (first == prev && cig_gap_in_run(a, a.blk[b], i, first, g.rpos, g.qpos)) atomicAdd(bad + 2, 1ull);
		}
	}
	__syncthreads();
	const bool wide = g.kind == CG_WALK && g.L > WALK_SERIAL;
	i32 cnt[4] = { 0, 0, 0, 0 };
	i32 n = 0;
	if (wide) { const int at = atomicAdd(&s_n, 1); s_list[at] = tid; s_prev[tid] = prev; s_slot[tid] = slot; s_col[tid] = col; }
	else if (g.kind == CG_BAD) { if (!EMIT) atomicAdd(bad, 1ull); }
	else if (g.kind != CG_NONE) n = cig_lane<EMIT, POS>(a, g, prev, run, slot, col, cnt);
	if (!EMIT) cig_totals(out, active, b, cnt);
	__syncthreads();
	const int nlist = s_n;
	for (int q = wv; q < nlist; q += 4) {
		// (the record's look-up is repeated by every lane of the wavefront: the addresses are uniform, so the loads are one request each)
		const int t = s_list[q];
		const i64 wt = (i64)blockIdx.x * 256 + t;
		const i32 bt = blk_last_le(a.blk, a.nb, &CigBlk::wbase, wt);
		const CigRec gt = cig_load(a, a.blk[bt].frag_off + (wt - a.blk[bt].wbase));
		i32 cw[4] = { 0, 0, 0, 0 };
		const i32 nt = cig_wave<EMIT, POS>(a, gt, s_prev[t], run, s_slot[t], s_col[t], cw);
		if (!EMIT) { cig_totals(out, true, bt, cw); if (lane == 0) s_val[t] = nt; }
	}
	if (EMIT) return;      // (safe: nothing below this line is reached on the EMIT path, so no __syncthreads is left waiting for these threads)
	__syncthreads();
	if (wide) n = s_val[tid];
	const i32 cols = (g.kind == CG_RUN || g.kind == CG_WALK) ? g.L : 0;
	if (active) { ns[w] = n; nc[w] = cols; }
	i64 ts = n, tc = cols;
	for (int d = 32; d; d >>= 1) { ts += __shfl_xor(ts, d); tc += __shfl_xor(tc, d); }
	if (lane == 0) { s_w[wv] = ts; s_w[4 + wv] = tc; }
	__syncthreads();
	if (tid == 0) { wg[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3]; wg[nwg + blockIdx.x] = s_w[4] + s_w[5] + s_w[6] + s_w[7]; }
}

// second level of the scan, two arrays: one workgroup turns the workgroups' sums into their first slots / first columns; the totals
// go behind the last record's prefix values and, with the count of records without a job, to the host's header
__global__ void __launch_bounds__(256) k_cig_scan(i64 nwg, i64 *wg, const unsigned long long *bad, i64 W, i64 *ps, i64 *pc, i64 *hdr)
{
	__shared__ i64 s_w[4];
	const i64 slots = wg_scan_sums(wg, nwg, s_w), cols = wg_scan_sums(wg + nwg, nwg, s_w);
	if (threadIdx.x == 0) { ps[W] = slots; pc[W] = cols; hdr[0] = slots; hdr[1] = cols; hdr[2] = (i64)bad[0]; }
}

// every record's first slot and first column: the workgroup's (k_cig_scan) plus the exclusive sums in front of it inside the workgroup
__global__ void __launch_bounds__(256) k_cig_prefix(i64 W, i64 nwg, const i32 *ns, const i32 *nc, const i64 *wg, i64 *ps, i64 *pc)
{
	__shared__ i64 s_w[8];
	const i64 w = (i64)blockIdx.x * 256 + threadIdx.x;
	i64 v[2] = { w < W ? ns[w] : 0, w < W ? nc[w] : 0 };
	wg_excl_scan(v, s_w);                           // (both arrays behind one barrier)
	if (w < W) { ps[w] = wg[blockIdx.x] + v[0]; pc[w] = wg[nwg + blockIdx.x] + v[1]; }
}

// a block's ops: from its first record's slot to the next block's
__global__ void k_cig_blocks(i32 nb, const CigBlk *blk, const i64 *ps, gsa_block_cigar *out)
{
	const i32 b = (i32)(blockIdx.x * blockDim.x + threadIdx.x);
	if (b >= nb) return;
	const i64 s0 = ps[blk[b].wbase], s1 = ps[blk[b + 1].wbase];
	out[b].cig_off = s0; out[b].n_cig = (i32)(s1 - s0); out[b]._pad = 0;
}

// run starts -> ops.  One work item per start; long[0] counts runs whose length does not fit an op's 28 bits
__global__ void __launch_bounds__(256) k_cig_pack(i32 nb, const CigBlk *blk, const gsa_block_cigar *out, const i64 *pc, const i64 *run, i64 n_ops, u32 *ops, unsigned long long *toolong)
{
	const i64 s = (i64)blockIdx.x * 256 + threadIdx.x;
	if (s >= n_ops) return;
	const i32 lo = blk_last_le(out, nb, &gsa_block_cigar::cig_off, s);      // (blocks without ops share their offset with the next one)
	const i64 off = out[lo].cig_off; const i32 n = out[lo].n_cig;
	const i64 k = s - off;
	if (k < 0 || k >= n) return;                    // (cannot happen: the blocks' ranges tile [0, n_ops))
	const i64 me = run[s];
	const i64 end = k + 1 < n ? (run[s + 1] >> 4) : pc[blk[lo + 1].wbase] - pc[blk[lo].wbase];
	const i64 len = end - (me >> 4);
	if (len <= 0 || len >= (1ll << 28)) atomicAdd(toolong, 1ull);
	ops[off + (blk[lo].bdir ? k : (i64)n - 1 - k)] = (u32)((u64)len << 4) | (u32)(me & 15);
}

int block_cigars(gsa_ctx *c, i32 k, gsa_cigars *out, bool pos)
{
	const ResultRange rr = result_range(c, k);
	const size_t nb = rr.nb;
	if (nb == 0 || c->n_frags <= 0) return GSA_OK;
	hipStream_t st = c->stream;
	if (!pin_ensure<CigBlk>(c, c->p_cblk, nb + 1) || !pin_ensure<i64>(c, c->p_chdr, 8) || !pin_ensure<gsa_block_cigar>(c, c->p_cout, nb)) return GSA_ERR_NOMEM;
	CigBlk *hb = c->p_cblk.as<CigBlk>(); i64 W = 0;
	for (size_t j = 0; j < nb; j++) {
		const gsa_block &bl = c->h_blocks[rr.b0 + j];
		const i32 nf = bl.n_frag > 0 ? bl.n_frag : 0;
		if (W + nf >= (1ll << 31) - 256) return gsa_fail(c, GSA_ERR_LIMIT, "gsa_block_cigars: too many records");
		CigBlk &v = hb[j]; v.frag_off = bl.frag_off + rr.f0; v.n_frag = nf; v.bdir = bl.bdir; v.wbase = (i32)W; v._pad = 0;
		W += nf;
	}
	{ CigBlk &v = hb[nb]; v.frag_off = 0; v.n_frag = 0; v.bdir = 1; v.wbase = (i32)W; v._pad = 0; }
	gsa_block_cigar *hout = c->p_cout.as<gsa_block_cigar>();
	if (W == 0) { memset(hout, 0, nb * sizeof(gsa_block_cigar)); out->n_blocks = (int32_t)nb; out->blk = hout; return GSA_OK; }
	const i64 nwg = (W + 255) / 256;
	ENS(CigBlk, d_cblk, nb + 1); ENS(gsa_block_cigar, d_cout, nb); ENS(i32, d_ccnt, 2 * ((size_t)W + 1)); ENS(i64, d_cwg, 2 * (size_t)nwg + 3); ENS(i64, d_cpre, 2 * ((size_t)W + 1));
	i32 *ns = c->d_ccnt.as<i32>(), *nc = ns + (W + 1);
	i64 *wg = c->d_cwg.as<i64>(); unsigned long long *bad = (unsigned long long *)(wg + 2 * nwg);      // {records without a job, runs too long for an op, pos: runs that go on in the next record somewhere else}
	i64 *ps = c->d_cpre.as<i64>(), *pc = ps + (W + 1);
	i64 *hdr = c->p_chdr.as<i64>();
	const CigBlk *dblk = c->d_cblk.as<CigBlk>(); gsa_block_cigar *dout = c->d_cout.as<gsa_block_cigar>();
	GSA_CHECK(c, hipMemcpyAsync(c->d_cblk.p, hb, (nb + 1) * sizeof(CigBlk), hipMemcpyHostToDevice, st));
	GSA_CHECK(c, hipMemsetAsync(dout, 0, nb * sizeof(gsa_block_cigar), st));
	GSA_CHECK(c, hipMemsetAsync(bad, 0, 3 * sizeof(unsigned long long), st));
	CigIn a;
	a.nb = (i32)nb; a.W = W; a.blk = dblk;
	gap_in_fill(c, a); a.n_out = 0; a.run_r = nullptr; a.run_q = nullptr;
	hipLaunchKernelGGL((k_cig_pass<false, false>), dim3((unsigned)nwg), dim3(256), 0, st, a, ns, nc, wg, nwg, bad, dout, (const i64 *)nullptr, (const i64 *)nullptr, (i64 *)nullptr);
	GSA_CHECK(c, hipGetLastError());
	hipLaunchKernelGGL(k_cig_scan, dim3(1), dim3(256), 0, st, nwg, wg, (const unsigned long long *)bad, W, ps, pc, hdr);
	GSA_CHECK(c, hipGetLastError());
	hipLaunchKernelGGL(k_cig_prefix, dim3((unsigned)nwg), dim3(256), 0, st, W, nwg, (const i32 *)ns, (const i32 *)nc, (const i64 *)wg, ps, pc);
	GSA_CHECK(c, hipGetLastError());
	hipLaunchKernelGGL(k_cig_blocks, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, st, (i32)nb, dblk, (const i64 *)ps, dout);
	GSA_CHECK(c, hipGetLastError());
	GSA_CHECK(c, hipMemcpyAsync(hout, dout, nb * sizeof(gsa_block_cigar), hipMemcpyDeviceToHost, st));
	GSA_CHECK(c, hipStreamSynchronize(st));
	const i64 n = hdr[0];
	if (hdr[2]) return gsa_fail(c, GSA_ERR_STATE, "internal: gsa_block_cigars met " + std::to_string((long long)hdr[2]) + " DP record(s) without a DP job");
	if (n >= (1ll << 31) - 256) return gsa_fail(c, GSA_ERR_LIMIT, "gsa_block_cigars: too many ops");
	if (n > 0) {
		// the output is sized from the scan's total; it goes home in one copy
		ENS(i64, d_crun, (size_t)n); ENS(u32, d_cops, (size_t)n); if (!pin_ensure<u32>(c, c->p_cops, (size_t)n)) return GSA_ERR_NOMEM;
		a.n_out = n;
		if (pos) {
			ENS(i64, d_crpos, (size_t)n); ENS(i32, d_cqpos, (size_t)n);
			a.run_r = c->d_crpos.as<i64>(); a.run_q = c->d_cqpos.as<i32>();
			hipLaunchKernelGGL((k_cig_pass<true, true>), dim3((unsigned)nwg), dim3(256), 0, st, a, ns, nc, wg, nwg, bad, dout, (const i64 *)ps, (const i64 *)pc, c->d_crun.as<i64>());
		} else
			hipLaunchKernelGGL((k_cig_pass<true, false>), dim3((unsigned)nwg), dim3(256), 0, st, a, ns, nc, wg, nwg, bad, dout, (const i64 *)ps, (const i64 *)pc, c->d_crun.as<i64>());
		GSA_CHECK(c, hipGetLastError());
		hipLaunchKernelGGL(k_cig_pack, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (i32)nb, dblk, (const gsa_block_cigar *)dout, (const i64 *)pc, (const i64 *)c->d_crun.as<i64>(), n, c->d_cops.as<u32>(), bad + 1);
		GSA_CHECK(c, hipGetLastError());
		GSA_CHECK(c, hipMemcpyAsync(c->p_cops.p, c->d_cops.p, (size_t)n * sizeof(u32), hipMemcpyDeviceToHost, st));
		GSA_CHECK(c, hipMemcpyAsync(hdr + 3, bad + 1, (pos ? 2 : 1) * sizeof(i64), hipMemcpyDeviceToHost, st));
		GSA_CHECK(c, hipStreamSynchronize(st));
		if (pos && hdr[4]) return gsa_fail(c, GSA_ERR_STATE, "internal: gsa_block_cs met " + std::to_string((long long)hdr[4]) + " run(s) that go on in the next record at another position");
		if (hdr[3]) return gsa_fail(c, GSA_ERR_LIMIT, "gsa_block_cigars: " + std::to_string((long long)hdr[3]) + " run(s) of 2^28 columns or more do not fit an op");
	}
	out->n_blocks = (int32_t)nb; out->n_ops = n; out->blk = hout; out->ops = n ? c->p_cops.as<u32>() : nullptr;
	return GSA_OK;
}
