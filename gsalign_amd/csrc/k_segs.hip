// gsalign_amd/csrc/k_segs.hip -- gsa_block_segs: every block of a stage-8 result as the {size, dt, dq} triples of a UCSC chain (include/gsa_hip.h), on the
// device, over what stage 8 and the CIGAR pass left there.  ("Chain" is the seed-chaining stage in this code base, k_chain.hip: the word here is SEGS.)
//
// A block's triples are a coarser run-length view of its columns than its CIGAR: '=' and 'X' runs merge into aligned SEGMENTS, 'I' and 'D' runs into the GAPS
// between them.  The CIGAR walk with its POS flag (k_cigar.hip) leaves, for every run start IN WALK ORDER, {column inside the block << 4 | class} (d_crun) and the
// reference and query position of that column (d_crpos / d_cqpos); the column of a block's first run is 0.  Everything else follows from those values, one work
// item per RUN, no column is looked at again:
//   segment start   an aligned run whose column is 0 or whose run in front is a gap run
//   gap start       a gap run (column > 0) whose run in front is aligned
//   COUNT   segment starts per workgroup
//   SCAN    one workgroup turns the workgroups' sums into their first segments; the total goes to the host, which sizes the rest from it
//   EMIT    the flags again, scanned inside the workgroup: every run gets the number of segment starts in front of it (pre[], the blocks' table is read off it);
//           a segment start stores its column and positions at its segment, a gap start the column where segment (starts so far - 1) ends, a block's last
//           run -- when it is aligned -- the block's column count as that end
//   PACK    one work item per segment: size = end column - start column (an aligned column holds one base of either side), dt / dq = the distance to the next
//           segment start on either side minus size (only positions of aligned columns are read: both sides hold a base there); stored at slot j of the
//           block, at n_seg - 1 - j with the gap IN FRONT for a reverse-strand block (k_cig_pack's rule)
// Integer arithmetic only, no atomics on the answer, no workgroup waits for another, nothing spins.  A gap run at column 0 (a block that starts in a gap: stage 8
// makes none) opens no segment and ends none: the triples start at the first aligned column, as a chain must.
#include <cstring>
#include "gsa_fm.h"
#include "gsa_walk.h"

struct SegIn {
	i64 n_ops, n_seg;                                                 // runs of the CIGAR pass; segments (COUNT: 0)
	const i64 *run; const i64 *run_r; const i32 *run_q;               // the CIGAR pass's run starts, walk order
	i32 nb; const CigBlk *blk; const gsa_block_cigar *cig; const i64 *pc;      // its block tables and the records' first columns (a block's column count)
	i32 *pre;                                                         // segment starts in front of every run, pre[n_ops] = n_seg
	i32 *s_col, *e_col; i64 *s_r; i32 *s_q;                           // per segment: first column, column behind its last, reference and query position of its first column
};

__device__ __forceinline__ bool seg_aligned(i64 run) { const i64 c = run & 15; return c == (i64)GSA_CIGAR_EQ || c == (i64)GSA_CIGAR_X; }
// run s opens a segment
__device__ __forceinline__ i32 seg_flag(const SegIn &a, i64 s, i64 me)
{
	if (!seg_aligned(me)) return 0;
	return ((me >> 4) == 0 || !seg_aligned(a.run[s - 1])) ? 1 : 0;    // (column > 0: the block has a run in front, s > 0)
}

__global__ void __launch_bounds__(256) k_seg_count(SegIn a, i64 *wg)
{
	__shared__ i64 s_w[4];
	const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
	const i64 s = (i64)blockIdx.x * 256 + tid;
	i64 t = s < a.n_ops ? seg_flag(a, s, a.run[s]) : 0;
	for (int d = 32; d; d >>= 1) t += __shfl_xor(t, d);
	if (lane == 0) s_w[wv] = t;
	__syncthreads();
	if (tid == 0) wg[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// second level: the workgroups' sums -> their first segments; the total goes behind the last run's prefix and to the host's header
__global__ void __launch_bounds__(256) k_seg_scan(i64 nwg, i64 *wg, i64 n, i32 *pre, i64 *hdr)
{
	__shared__ i64 s_w[4];
	const i64 total = wg_scan_sums(wg, nwg, s_w);
	if (threadIdx.x == 0) { pre[n] = total < (1ll << 31) ? (i32)total : 0x7fffffff; hdr[0] = total; }
}

__global__ void __launch_bounds__(256) k_seg_emit(SegIn a, const i64 *wg)
{
	__shared__ i32 s_w[4];
	const i64 s = (i64)blockIdx.x * 256 + threadIdx.x;
	const bool in = s < a.n_ops;
	const i64 me = in ? a.run[s] : 0;
	const i32 f = in ? seg_flag(a, s, me) : 0;
	const i64 ex = wg[blockIdx.x] + (i64)wg_excl_scan<i32>(f, s_w);
	if (!in) return;
	a.pre[s] = (i32)ex;
	const i64 col = me >> 4;
	const bool al = seg_aligned(me);
	const i64 j = f ? ex : ex - 1;                                    // the segment this run opens, or the one the runs in front of it belong to
	if (f && j < a.n_seg) { a.s_col[j] = (i32)col; a.s_r[j] = a.run_r[s]; a.s_q[j] = a.run_q[s]; }
	if (!al && col > 0 && seg_aligned(a.run[s - 1]) && j >= 0 && j < a.n_seg) a.e_col[j] = (i32)col;
	if (al && (s + 1 == a.n_ops || (a.run[s + 1] >> 4) == 0) && j >= 0 && j < a.n_seg) {      // the block's last run: its segment ends with the block
		const i32 b = blk_last_le(a.cig, a.nb, &gsa_block_cigar::cig_off, s);      // (blocks without ops share their offset with the next one)
		a.e_col[j] = (i32)(a.pc[a.blk[b + 1].wbase] - a.pc[a.blk[b].wbase]);
	}
}

// a block's segments: from the prefix at its first run to the prefix at the next block's (the blocks' run ranges tile [0, n_ops))
__global__ void k_seg_blocks(i32 nb, i64 n_ops, const gsa_block_cigar *cig, const i32 *pre, gsa_seg_block *out)
{
	const i32 b = (i32)(blockIdx.x * blockDim.x + threadIdx.x);
	if (b >= nb) return;
	i64 o0 = cig[b].cig_off, o1 = o0 + cig[b].n_cig;
	if (o0 < 0) o0 = 0; if (o0 > n_ops) o0 = n_ops; if (o1 < o0) o1 = o0; if (o1 > n_ops) o1 = n_ops;      // (cannot happen: pre[] has n_ops + 1 entries)
	out[b].seg_off = pre[o0]; out[b].n_seg = pre[o1] - pre[o0]; out[b]._pad = 0;
}

// boundaries -> triples.  bad[0] counts triples that are no chain line: a size below 1, a gap with a negative side or with nothing in it
__global__ void __launch_bounds__(256) k_seg_pack(SegIn a, const gsa_seg_block *out, gsa_seg *seg, unsigned long long *bad)
{
	const i64 j = (i64)blockIdx.x * 256 + threadIdx.x;
	if (j >= a.n_seg) return;
	const i32 lo = blk_last_le(out, a.nb, &gsa_seg_block::seg_off, j);      // (blocks without segments share their offset with the next one)
	const i64 off = out[lo].seg_off; const i64 n = out[lo].n_seg;
	const i64 k = j - off;
	if (k < 0 || k >= n) return;                                     // (cannot happen: the blocks' ranges tile [0, n_seg))
	const bool fwd = a.blk[lo].bdir != 0;
	gsa_seg t;
	t.size = a.e_col[j] - a.s_col[j]; t.dt = 0; t.dq = 0;
	// the gap printed behind this segment: the one behind it in walk order, for a reverse-strand block the one in front of it
	const i64 g = fwd ? j : j - 1;
	const bool has = fwd ? k + 1 < n : k > 0;
	if (has) { const i32 sz = a.e_col[g] - a.s_col[g]; t.dt = (i32)(a.s_r[g + 1] - a.s_r[g]) - sz; t.dq = a.s_q[g + 1] - a.s_q[g] - sz; }
	if (t.size < 1 || (has && (t.dt < 0 || t.dq < 0 || (t.dt | t.dq) == 0))) atomicAdd(bad, 1ull);
	seg[off + (fwd ? k : n - 1 - k)] = t;
}

int block_segs(gsa_ctx *c, i32 k, gsa_segs *out, gsa_cigars *cig_out, const gsa_cigars *have)
{
	gsa_cigars cig = { 0, 0, nullptr, nullptr };
	if (have) cig = *have;                                            // (gsa_align_many_ex behind gsa_block_cs: the walk with positions has just run for this contig)
	else { const int rc_cig = block_cigars(c, k, &cig, true); if (cig_out) *cig_out = cig; if (rc_cig) return rc_cig; }
	const size_t nb = (size_t)cig.n_blocks; const i64 n = cig.n_ops;
	if (nb == 0) return GSA_OK;
	hipStream_t st = c->stream;
	if (!pin_ensure<gsa_seg_block>(c, c->p_sgout, nb) || !pin_ensure<i64>(c, c->p_sghdr, 4)) return GSA_ERR_NOMEM;
	gsa_seg_block *hout = c->p_sgout.as<gsa_seg_block>();
	if (n == 0) { memset(hout, 0, nb * sizeof(gsa_seg_block)); out->n_blocks = (int32_t)nb; out->blk = hout; return GSA_OK; }
	const i64 nwg = (n + 255) / 256;
	ENS(i64, d_sgwg, (size_t)nwg + 1); ENS(i32, d_sgpre, (size_t)n + 1); ENS(gsa_seg_block, d_sgout, nb);
	i64 *wg = c->d_sgwg.as<i64>(), *hdr = c->p_sghdr.as<i64>();
	unsigned long long *bad = (unsigned long long *)(wg + nwg);
	SegIn a;
	a.n_ops = n; a.n_seg = 0;
	a.run = c->d_crun.as<i64>(); a.run_r = c->d_crpos.as<i64>(); a.run_q = c->d_cqpos.as<i32>();
	a.nb = (i32)nb; a.blk = c->d_cblk.as<CigBlk>(); a.cig = c->d_cout.as<gsa_block_cigar>();
	a.pc = c->d_cpre.as<i64>() + ((i64)c->p_cblk.as<CigBlk>()[nb].wbase + 1);      // (block_cigars: ps[W + 1] | pc[W + 1])
	a.pre = c->d_sgpre.as<i32>();
	a.s_col = a.e_col = a.s_q = nullptr; a.s_r = nullptr;
	GSA_CHECK(c, hipMemsetAsync(bad, 0, sizeof(unsigned long long), st));
	hipLaunchKernelGGL(k_seg_count, dim3((unsigned)nwg), dim3(256), 0, st, a, wg);
	GSA_CHECK(c, hipGetLastError());
	hipLaunchKernelGGL(k_seg_scan, dim3(1), dim3(256), 0, st, nwg, wg, n, a.pre, hdr);
	GSA_CHECK(c, hipGetLastError());
	GSA_CHECK(c, hipStreamSynchronize(st));
	const i64 total = hdr[0];
	if (total >= (1ll << 31) - 256) return gsa_fail(c, GSA_ERR_LIMIT, "gsa_block_segs: too many segments");
	// the boundaries and the triples are sized from the scan's total; blocks and triples go home in one copy each
	const size_t m = (size_t)(total > 0 ? total : 1);
	ENS(i64, d_sgbnd, 3 * m); ENS(gsa_seg, d_sgseg, m); if (!pin_ensure<gsa_seg>(c, c->p_sgseg, m)) return GSA_ERR_NOMEM;
	a.n_seg = total;
	a.s_r = c->d_sgbnd.as<i64>(); a.s_col = (i32 *)(a.s_r + m); a.e_col = a.s_col + m; a.s_q = a.e_col + m;      // (20 bytes per segment)
	hipLaunchKernelGGL(k_seg_emit, dim3((unsigned)nwg), dim3(256), 0, st, a, (const i64 *)wg);
	GSA_CHECK(c, hipGetLastError());
	hipLaunchKernelGGL(k_seg_blocks, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, st, (i32)nb, n, a.cig, (const i32 *)a.pre, c->d_sgout.as<gsa_seg_block>());
	GSA_CHECK(c, hipGetLastError());
	GSA_CHECK(c, hipMemcpyAsync(hout, c->d_sgout.p, nb * sizeof(gsa_seg_block), hipMemcpyDeviceToHost, st));
	if (total > 0) {
		hipLaunchKernelGGL(k_seg_pack, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a, (const gsa_seg_block *)c->d_sgout.as<gsa_seg_block>(), c->d_sgseg.as<gsa_seg>(), bad);
		GSA_CHECK(c, hipGetLastError());
		GSA_CHECK(c, hipMemcpyAsync(c->p_sgseg.p, c->d_sgseg.p, (size_t)total * sizeof(gsa_seg), hipMemcpyDeviceToHost, st));
	}
	GSA_CHECK(c, hipMemcpyAsync(hdr + 1, bad, sizeof(i64), hipMemcpyDeviceToHost, st));
	GSA_CHECK(c, hipStreamSynchronize(st));
	if (hdr[1]) return gsa_fail(c, GSA_ERR_STATE, "internal: gsa_block_segs met " + std::to_string((long long)hdr[1]) + " segment(s) or gap(s) that are no chain line");
	out->n_blocks = (int32_t)nb; out->n_segs = total; out->blk = hout; out->seg = total ? c->p_sgseg.as<gsa_seg>() : nullptr;
	return GSA_OK;
}
