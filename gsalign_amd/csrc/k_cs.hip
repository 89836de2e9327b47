// gsalign_amd/csrc/k_cs.hip -- gsa_block_cs: the cs string (minimap2's cs:Z:, short form; include/gsa_hip.h) of every block of a stage-8 result, on the
// device, over what stage 8 and the CIGAR pass left there.
//
// A block's cs is a function of its CIGAR ops, in output order, and of the bases under them: '=' n -> ":n", 'X' n -> n groups "*rq", 'I' n -> "+" and the n
// query letters, 'D' n -> "-" and the n reference letters.  The ops alone carry no positions, so the CIGAR walk runs with its POS flag (k_cigar.hip): beside
// run[slot] it leaves the reference and query position of the run's first column IN WALK ORDER (d_crpos / d_cqpos), and it refuses a result in which a run
// other than '=' goes on in the next record somewhere else -- inside a run the bases are then consecutive on either side.  Three passes of one work item per op:
//   LEN     bytes per op (1 + decimal digits | 3 n | 1 + n), per workgroup
//   SCAN    one workgroup turns the workgroups' sums into their first bytes, PREFIX gives every op its own (64 bit); BLOCKS: a block's string runs from its
//           first op's byte to the next block's
//   EMIT    an op of at most CS_SERIAL columns is written by one lane, a longer one by a whole wavefront, 64 columns per step (a lane's bytes lie behind its
//           lower neighbour's).  Output char i of an op of a reverse-strand block is walk column n - 1 - i, complemented.  Every store is checked against the
//           scan's total, every base's position against the text it is read from.
// No workgroup waits for another, nothing spins.
#include <cstring>
#include "gsa_fm.h"
#include "gsa_walk.h"

#define CS_SERIAL 64

struct CsIn {
	i32 nb; i64 n_ops, n_bytes;
	const CigBlk *blk; const gsa_block_cigar *cig;                    // the CIGAR pass's block tables (in: strand; out: first op, ops)
	const u32 *ops; const i64 *po;                                    // ops in output order; first byte of every op, po[n_ops] = n_bytes
	const i64 *run_r; const i32 *run_q;                               // first position of every run, in WALK order (slot = run index)
	const uint8_t *query, *ref; i64 qry_n, ref_n;
	char *cs; unsigned long long *bad;                                // bad[0]: blocks of 2^31 bytes or more, bad[1]: bases asked for outside their text
};

__device__ __forceinline__ i32 cs_digits(u32 v) { i32 n = 1; while (v >= 10u) { v /= 10u; n++; } return n; }
__device__ __forceinline__ i64 cs_op_bytes(u32 op)
{
	const u32 L = op >> 4, cls = op & 15u;
	return cls == GSA_CIGAR_EQ ? 1 + (i64)cs_digits(L) : (cls == GSA_CIGAR_X ? 3 * (i64)L : 1 + (i64)L);
}

__global__ void __launch_bounds__(256) k_cs_len(i64 n, const u32 *ops, i64 *len, i64 *wg)
{
	__shared__ i64 s_w[4];
	const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
	const i64 s = (i64)blockIdx.x * 256 + tid;
	const i64 v = s < n ? cs_op_bytes(ops[s]) : 0;
	if (s < n) len[s] = v;
	i64 t = v;
	for (int d = 32; d; d >>= 1) t += __shfl_xor(t, d);
	if (lane == 0) s_w[wv] = t;
	__syncthreads();
	if (tid == 0) wg[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// second level: the workgroups' sums -> their first bytes; the total goes behind the last op's offset and to the host's header
__global__ void __launch_bounds__(256) k_cs_scan(i64 nwg, i64 *wg, i64 n, i64 *po, i64 *hdr)
{
	__shared__ i64 s_w[4];
	const i64 total = wg_scan_sums(wg, nwg, s_w);
	if (threadIdx.x == 0) { po[n] = total; hdr[0] = total; }
}

__global__ void __launch_bounds__(256) k_cs_prefix(i64 n, const i64 *len, const i64 *wg, i64 *po)
{
	__shared__ i64 s_w[4];
	const i64 s = (i64)blockIdx.x * 256 + threadIdx.x;
	const i64 e = wg_excl_scan<i64>(s < n ? len[s] : 0, s_w);
	if (s < n) po[s] = wg[blockIdx.x] + e;
}

// a block's string: from its first op's byte to the byte behind its last op (the blocks' op ranges tile [0, n_ops), so that is the next block's first byte)
__global__ void k_cs_blocks(i32 nb, i64 n_ops, const gsa_block_cigar *cig, const i64 *po, gsa_cs_block *out, unsigned long long *bad)
{
	const i32 b = (i32)(blockIdx.x * blockDim.x + threadIdx.x);
	if (b >= nb) return;
	i64 o0 = cig[b].cig_off, o1 = o0 + cig[b].n_cig;
	if (o0 < 0) o0 = 0; if (o0 > n_ops) o0 = n_ops; if (o1 < o0) o1 = o0; if (o1 > n_ops) o1 = n_ops;      // (cannot happen: po[] has n_ops + 1 entries)
	const i64 n = po[o1] - po[o0];
	if (n >= (1ll << 31)) atomicAdd(bad, 1ull);
	out[b].cs_off = po[o0]; out[b].n_cs = (int32_t)n; out[b]._pad = 0;
}

struct CsOp { i64 at, rp; i32 qp; u32 L, cls; bool fwd; };           // first byte, first positions in walk order, columns, class, strand

__device__ CsOp cs_load(const CsIn &a, i64 s)
{
	CsOp o;
	const i32 lo = blk_last_le(a.cig, a.nb, &gsa_block_cigar::cig_off, s);      // (blocks without ops share their offset with the next one)
	const i64 off = a.cig[lo].cig_off; const i64 n = a.cig[lo].n_cig;
	const u32 op = a.ops[s];
	o.fwd = a.blk[lo].bdir != 0; o.L = op >> 4; o.cls = op & 15u; o.at = a.po[s];
	i64 k = s - off; if (k < 0 || k >= n) { o.L = 0; k = 0; }        // (cannot happen: the blocks' ranges tile [0, n_ops))
	const i64 slot = off + (o.fwd ? k : n - 1 - k);                 // k_cig_pack stores run k of a reverse-strand block at n - 1 - k
	o.rp = 0; o.qp = 0;
	if (o.cls != GSA_CIGAR_EQ && slot >= 0 && slot < a.n_ops) { o.rp = a.run_r[slot]; o.qp = a.run_q[slot]; }
	return o;
}

__device__ __forceinline__ void cs_put(const CsIn &a, i64 at, char ch) { if (at >= 0 && at < a.n_bytes) a.cs[at] = ch; }
// "acgtn"[nt4(b)], for a reverse-strand block "tgcan"[nt4(b)]
__device__ __forceinline__ char cs_letter(uint8_t b, bool fwd) { return (char)((fwd ? 0x6e74676361ull : 0x6e61636774ull) >> (8 * gsa_nt4(b))); }
__device__ __forceinline__ uint8_t cs_ref(const CsIn &a, i64 p) { if (p >= 0 && p < a.ref_n) return a.ref[p]; atomicAdd(a.bad + 1, 1ull); return (uint8_t)'N'; }
__device__ __forceinline__ uint8_t cs_qry(const CsIn &a, i64 p) { if (p >= 0 && p < a.qry_n) return a.query[p]; atomicAdd(a.bad + 1, 1ull); return (uint8_t)'N'; }

// output column i of an op that is not '='
__device__ __forceinline__ void cs_column(const CsIn &a, const CsOp &o, u32 i)
{
	const i64 d = o.fwd ? (i64)i : (i64)o.L - 1 - (i64)i;            // its column in walk order
	if (o.cls == GSA_CIGAR_X) {
		const i64 at = o.at + 3 * (i64)i;
		cs_put(a, at, '*'); cs_put(a, at + 1, cs_letter(cs_ref(a, o.rp + d), o.fwd)); cs_put(a, at + 2, cs_letter(cs_qry(a, (i64)o.qp + d), o.fwd));
	} else if (o.cls == GSA_CIGAR_INS) cs_put(a, o.at + 1 + (i64)i, cs_letter(cs_qry(a, (i64)o.qp + d), o.fwd));
	else cs_put(a, o.at + 1 + (i64)i, cs_letter(cs_ref(a, o.rp + d), o.fwd));
}

__global__ void __launch_bounds__(256) k_cs_emit(CsIn a)
{
	__shared__ i32 s_list[256];
	__shared__ int s_n;
	const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
	const i64 s = (i64)blockIdx.x * 256 + tid;
	if (tid == 0) s_n = 0;
	__syncthreads();
	if (s < a.n_ops) {
		const CsOp o = cs_load(a, s);
		if (o.cls == GSA_CIGAR_EQ) {
			char tmp[12]; int m = 0; u32 v = o.L;
			do { tmp[m++] = (char)('0' + v % 10u); v /= 10u; } while (v);
			cs_put(a, o.at, ':');
			for (int k = 0; k < m; k++) cs_put(a, o.at + 1 + k, tmp[m - 1 - k]);
		} else if (o.L > 0) {
			if (o.cls != GSA_CIGAR_X) cs_put(a, o.at, o.cls == GSA_CIGAR_INS ? '+' : '-');
			if (o.L <= CS_SERIAL) { for (u32 i = 0; i < o.L; i++) cs_column(a, o, i); }
			else { const int at = atomicAdd(&s_n, 1); s_list[at] = tid; }
		}
	}
	__syncthreads();
	const int nlist = s_n;
	for (int q = wv; q < nlist; q += 4) {
		// (the op's look-up is repeated by every lane of the wavefront: the addresses are uniform)
		const CsOp o = cs_load(a, (i64)blockIdx.x * 256 + s_list[q]);
		for (u32 base = 0; base < o.L; base += 64) { const u32 i = base + (u32)lane; if (i < o.L) cs_column(a, o, i); }
	}
}

int block_cs(gsa_ctx *c, i32 k, gsa_cs *out, gsa_cigars *cig_out)
{
	gsa_cigars cig = { 0, 0, nullptr, nullptr };
	const int rc_cig = block_cigars(c, k, &cig, true);
	if (cig_out) *cig_out = cig;
	if (rc_cig) return rc_cig;
	const size_t nb = (size_t)cig.n_blocks; const i64 n = cig.n_ops;
	if (nb == 0) return GSA_OK;
	hipStream_t st = c->stream;
	if (!pin_ensure<gsa_cs_block>(c, c->p_sout, nb) || !pin_ensure<i64>(c, c->p_shdr, 4)) return GSA_ERR_NOMEM;
	gsa_cs_block *hout = c->p_sout.as<gsa_cs_block>();
	if (n == 0) { memset(hout, 0, nb * sizeof(gsa_cs_block)); out->n_blocks = (int32_t)nb; out->blk = hout; return GSA_OK; }
	const i64 nwg = (n + 255) / 256;
	ENS(i64, d_slen, (size_t)n); ENS(i64, d_swg, (size_t)nwg + 2); ENS(i64, d_spre, (size_t)n + 1); ENS(gsa_cs_block, d_sout, nb);
	i64 *len = c->d_slen.as<i64>(), *wg = c->d_swg.as<i64>(), *po = c->d_spre.as<i64>(), *hdr = c->p_shdr.as<i64>();
	unsigned long long *bad = (unsigned long long *)(wg + nwg);
	const u32 *ops = c->d_cops.as<u32>(); const gsa_block_cigar *dcig = c->d_cout.as<gsa_block_cigar>();
	GSA_CHECK(c, hipMemsetAsync(bad, 0, 2 * sizeof(unsigned long long), st));
	hipLaunchKernelGGL(k_cs_len, dim3((unsigned)nwg), dim3(256), 0, st, n, ops, len, wg);
	GSA_CHECK(c, hipGetLastError());
	hipLaunchKernelGGL(k_cs_scan, dim3(1), dim3(256), 0, st, nwg, wg, n, po, hdr);
	GSA_CHECK(c, hipGetLastError());
	hipLaunchKernelGGL(k_cs_prefix, dim3((unsigned)nwg), dim3(256), 0, st, n, (const i64 *)len, (const i64 *)wg, po);
	GSA_CHECK(c, hipGetLastError());
	hipLaunchKernelGGL(k_cs_blocks, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, st, (i32)nb, n, dcig, (const i64 *)po, c->d_sout.as<gsa_cs_block>(), bad);
	GSA_CHECK(c, hipGetLastError());
	GSA_CHECK(c, hipMemcpyAsync(hout, c->d_sout.p, nb * sizeof(gsa_cs_block), hipMemcpyDeviceToHost, st));
	GSA_CHECK(c, hipMemcpyAsync(hdr + 1, bad, sizeof(i64), hipMemcpyDeviceToHost, st));
	GSA_CHECK(c, hipStreamSynchronize(st));
	const i64 total = hdr[0];
	if (hdr[1]) return gsa_fail(c, GSA_ERR_LIMIT, "gsa_block_cs: " + std::to_string((long long)hdr[1]) + " block(s) with a string of 2^31 bytes or more");
	if (total > 0) {
		// the output is sized from the scan's total; it goes home in one copy
		ENS(char, d_cs, (size_t)total); if (!pin_ensure<char>(c, c->p_cs, (size_t)total)) return GSA_ERR_NOMEM;
		CsIn a;
		a.nb = (i32)nb; a.n_ops = n; a.n_bytes = total;
		a.blk = c->d_cblk.as<CigBlk>(); a.cig = dcig; a.ops = ops; a.po = po;
		a.run_r = c->d_crpos.as<i64>(); a.run_q = c->d_cqpos.as<i32>();
		a.query = c->q_dev; a.ref = c->di.ref;
		a.qry_n = (c->bnd.n && !c->b_off.empty()) ? (i64)c->b_off.back() : (i64)c->qlen; a.ref_n = 2 * c->G;
		a.cs = c->d_cs.as<char>(); a.bad = bad;
		hipLaunchKernelGGL(k_cs_emit, dim3((unsigned)nwg), dim3(256), 0, st, a);
		GSA_CHECK(c, hipGetLastError());
		GSA_CHECK(c, hipMemcpyAsync(c->p_cs.p, c->d_cs.p, (size_t)total, hipMemcpyDeviceToHost, st));
		GSA_CHECK(c, hipMemcpyAsync(hdr + 2, bad + 1, sizeof(i64), hipMemcpyDeviceToHost, st));
		GSA_CHECK(c, hipStreamSynchronize(st));
		if (hdr[2]) return gsa_fail(c, GSA_ERR_STATE, "internal: gsa_block_cs asked for " + std::to_string((long long)hdr[2]) + " base(s) outside the reference or the query");
	}
	out->n_blocks = (int32_t)nb; out->n_bytes = total; out->blk = hout; out->cs = total ? c->p_cs.as<char>() : nullptr;
	return GSA_OK;
}
