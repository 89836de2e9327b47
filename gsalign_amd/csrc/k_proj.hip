// gsalign_amd/csrc/k_proj.hip -- gsa_project: the query projected onto the reference (include/gsa_hip.h), on the device, over what stage 8 left there.
//
// The accumulator is one u32 per forward reference position; every covered column of every painted block offers key | code to its word with an integer atomicMax, so
// the array does not depend on the order in which blocks, contigs, contexts and devices arrive.  One work item per record of the painted blocks for the bookkeeping, one
// lane per COLUMN for the painting: seeds are ~99 % of the records and hold nearly all columns, and one identical stretch is a single seed of megabases.
//   PREFIX  per record: its trimmed reference length if it is a run record (seed, equal-length gap without DP, pure deletion), else 0 -> exclusive prefix inside the
//           workgroup, sums per workgroup; SCAN turns the sums into the workgroups' first columns and leaves the total behind the last record; ADD makes the prefix global
//   RUNS    a workgroup per PROJ_TILE columns of that prefix, a lane per column: two searches per tile (its first and last record, uniform addresses), a search between
//           them per lane -- repeated only when the lane's next column has left its record -- then the query byte and the atomicMax.  Neighbouring lanes read neighbouring
//           query bytes and hit neighbouring words: 256 contiguous bytes per wave instruction, ascending on the forward strand, descending on the reverse strand.  The
//           grid is sized by the host-known sum of the blocks' spans (no read-back of the total); tiles beyond the device total leave.
//           (A walk forward from the tile's first record was the first sketch; the bounded search costs the same six steps whether the tile holds two records or two hundred.)
//   GAPS    a work item per record again, DP-gap records only: at most WALK_SERIAL columns by their lane, longer ones by a wavefront in 64-column steps
//   TEXT    words -> characters, 16 per lane, one 16-byte store;  MERGE  host words into the array, the maximum stays
// No workgroup waits for another, nothing spins; every atomic's index is checked against G; the query is read for covered columns only and the reference text not at all
// (a column's character is the query's).  As in the other passes the columns of a DP gap come from the op string of its DP job (gsa_walk.h), never from the string pools.
#include "gsa_walk.h"

#define PROJ_TILE 2048        // columns per workgroup of k_proj_runs: eight per lane
#define PROJ_CHUNK ((i64)1 << 22)      // positions per staging round of fetch and merge: 16 MB of words

// one painted block (gsa_walk.h's span table entry, unsorted) and the key its columns offer
struct ProjBlk : SpanBlk { u32 key; i32 _pad; };
struct ProjIn : GapIn {
	const ProjBlk *blk; i32 nb;
	i64 W, G;
	i32 qtot;                                                    // bases the device copy of the contig (a bundle: the concatenation) holds
	u32 *acc;
};
// cnt[0]: DP records without a DP job, cnt[1]: columns outside their record or sequence -- neither can happen; both are counted and reported, never skipped silently; cnt[2]: gap columns offered
enum { PJ_NOJOB = 0, PJ_OUT = 1, PJ_GAPCOLS = 2, PJ_NCNT = 3 };

__device__ __forceinline__ u32 proj_code(uint8_t q) { return (u32)gsa_nt4(q) + 1u; }      // 1..4 acgtACGT, 5 anything else

__device__ __forceinline__ void proj_offer(const ProjIn &a, const ProjBlk &b, i64 t, u32 code, unsigned long long *cnt)
{
	const i64 p = b.rev ? 2 * a.G - 1 - t : t;
	if (p < 0 || p >= a.G) { atomicAdd(cnt + PJ_OUT, 1ull); return; }
	atomicMax(a.acc + p, b.key | ((b.rev && code <= 4u) ? 5u - code : code));
}

// the record of work item w and its block
struct ProjRec { ProjBlk b; gsa_frag f; i32 ftype; i64 i; };
__device__ __forceinline__ ProjRec proj_rec(const ProjIn &a, i64 w)
{
	ProjRec x;
	x.b = a.blk[blk_last_le(a.blk, a.nb, &SpanBlk::wbase, w)];
	x.i = x.b.frag_off + (w - x.b.wbase);
	x.f = a.frag[x.i]; x.ftype = a.ftype[x.i];
	return x;
}
// a run record: its columns are known without a walk -- a seed, an equal-length gap that needed no DP, a pure deletion
__device__ __forceinline__ bool proj_is_run(const ProjRec &x)
{
	if (x.ftype == FT_SEED) return x.f.qlen > 0;
	return x.f.rlen > 0 && (x.f.qlen <= 0 || x.ftype != FT_DP);
}
// the part of the record's reference bases the block's trimmed span holds: [lo, lo + n)
__device__ __forceinline__ i64 proj_span(const ProjRec &x, i64 &lo)
{
	lo = x.f.rpos > x.b.start ? x.f.rpos : x.b.start;
	const i64 hi = x.f.rpos + x.f.rlen < x.b.end ? x.f.rpos + x.f.rlen : x.b.end;
	return hi > lo ? hi - lo : 0;
}

__global__ void __launch_bounds__(256) k_proj_prefix(ProjIn a, i64 *pre, i64 *wg)
{
	__shared__ i64 s_w[4];
	const i64 w = (i64)blockIdx.x * 256 + threadIdx.x;
	i64 v = 0;
	if (w < a.W) { const ProjRec x = proj_rec(a, w); i64 lo; if (proj_is_run(x)) v = proj_span(x, lo); }
	const i64 e = wg_excl_scan<i64>(v, s_w);
	if (w < a.W) pre[w] = e;
	if (threadIdx.x == 255) wg[blockIdx.x] = e + v;
}
__global__ void __launch_bounds__(256) k_proj_add(i64 W, i64 *pre, const i64 *wg)
{
	const i64 w = (i64)blockIdx.x * 256 + threadIdx.x;
	if (w < W) pre[w] += wg[blockIdx.x];
}

// the last of pre[lo .. hi) that is <= x (pre[lo] <= x)
__device__ __forceinline__ i64 proj_last_le(const i64 *pre, i64 lo, i64 hi, i64 x)
{
	while (hi - lo > 1) { const i64 m = (lo + hi) >> 1; if (pre[m] <= x) lo = m; else hi = m; }
	return lo;
}

__global__ void __launch_bounds__(256) k_proj_runs(ProjIn a, const i64 *pre, unsigned long long *cnt)
{
	const i64 total = pre[a.W];
	const i64 c0 = (i64)blockIdx.x * PROJ_TILE;
	if (c0 >= total) return;
	const i64 c1 = c0 + PROJ_TILE < total ? c0 + PROJ_TILE : total;
	// (uniform addresses: the two searches are one request per step for the whole workgroup)
	const i64 r_lo = proj_last_le(pre, 0, a.W, c0), r_hi = proj_last_le(pre, r_lo, a.W, c1 - 1);
	ProjRec x; i64 r_beg = 0, r_end = -1, lo = 0;      // the lane's current record holds columns [r_beg, r_end) of the prefix; its first covered base is lo
	for (i64 c = c0 + threadIdx.x; c < c1; c += 256) {
		if (c >= r_end) {
			const i64 r = proj_last_le(pre, r_lo, r_hi + 1, c);
			x = proj_rec(a, r);
			r_beg = pre[r]; r_end = r_beg + proj_span(x, lo);
			if (c >= r_end) { atomicAdd(cnt + PJ_OUT, 1ull); r_end = -1; continue; }      // (the prefix and the record disagree)
		}
		const i64 t = lo + (c - r_beg);
		u32 code = 6u;
		if (x.f.qlen > 0) {
			const i64 d = t - x.f.rpos, qp = (i64)x.f.qpos + d;
			if (d >= (i64)x.f.qlen || qp < 0 || qp >= (i64)a.qtot) { atomicAdd(cnt + PJ_OUT, 1ull); continue; }
			code = proj_code(a.query[qp]);
		}
		proj_offer(a, x.b, t, code, cnt);
	}
}

// the columns of a gap of at most WALK_SERIAL ops (op[0 .. L)), by one lane; returns the columns offered.  'D' puts '-' into the reference row (no reference base), 'I'
// into the query row (code 6), 'M' pairs a base of either side
__device__ i32 proj_lane(const ProjIn &a, const ProjRec &x, const uint8_t *op, i32 L, unsigned long long *cnt)
{
	i64 rp = x.f.rpos; i32 qp = x.f.qpos, n = 0; bool ok = true;
	const i64 rend = x.f.rpos + x.f.rlen;
	for (i32 i = 0; i < L; i++) {
		const int ch = (int)op[i];
		if (ch != 'D') {
			if (rp >= rend) ok = false;
			else if (rp >= x.b.start && rp < x.b.end) {
				u32 code = 6u;
				if (ch != 'I') { if (qp - x.f.qpos >= x.f.qlen || qp < 0 || qp >= a.qtot) { ok = false; code = 0u; } else code = proj_code(a.query[qp]); }
				if (code) { proj_offer(a, x.b, rp, code, cnt); n++; }
			}
		}
		col_advance(ch, rp, qp);
	}
	if (rp != rend) ok = false;      // (the ops hold fewer reference bases than the record)
	if (!ok) atomicAdd(cnt + PJ_OUT, 1ull);
	return n;
}

// the same by a whole wavefront, 64 columns per step (wave_step); returns the lane's own offered columns
__device__ i32 proj_wave(const ProjIn &a, const ProjRec &x, const uint8_t *op, i32 L, unsigned long long *cnt)
{
	const int lane = threadIdx.x & 63;
	i64 rp0 = x.f.rpos; i32 qp0 = x.f.qpos, n = 0; bool ok = true;
	const i64 rend = x.f.rpos + x.f.rlen;
	for (i32 base = 0; base < L; base += 64) {
		const WaveCol w = wave_step(op, L, base, rp0, qp0);
		if (w.c1) {
			if (w.rp >= rend) ok = false;
			else if (w.rp >= x.b.start && w.rp < x.b.end) {
				u32 code = 6u;
				if (w.ch == 'M') { if (w.qp - x.f.qpos >= x.f.qlen || w.qp < 0 || w.qp >= a.qtot) { ok = false; code = 0u; } else code = proj_code(a.query[w.qp]); }
				if (code) { proj_offer(a, x.b, w.rp, code, cnt); n++; }
			}
		}
	}
	if (rp0 != rend) ok = false;
	if (__ballot(!ok) && lane == 0) atomicAdd(cnt + PJ_OUT, 1ull);
	return n;
}

__global__ void __launch_bounds__(256) k_proj_gaps(ProjIn a, unsigned long long *cnt)
{
	__shared__ i32 s_list[256];
	__shared__ int s_n;
	const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
	const i64 w = (i64)blockIdx.x * 256 + tid;
	if (tid == 0) s_n = 0;
	__syncthreads();
	i32 n = 0;
	if (w < a.W) {
		const ProjRec x = proj_rec(a, w);
		if (x.ftype == FT_DP && x.f.qlen > 0 && x.f.rlen > 0) {
			const uint8_t *op = nullptr; i32 L = 0;
			if (!gap_ops(a, x.i, x.ftype, x.f, op, L) || !op) atomicAdd(cnt + PJ_NOJOB, 1ull);
			else if (L > WALK_SERIAL) s_list[atomicAdd(&s_n, 1)] = tid;
			else n = proj_lane(a, x, op, L, cnt);
		}
	}
	__syncthreads();
	const int nlist = s_n;
	for (int q = wv; q < nlist; q += 4) {
		// (the record's look-up is repeated by every lane of the wavefront: the addresses are uniform, so the loads are one request each)
		const ProjRec x = proj_rec(a, (i64)blockIdx.x * 256 + s_list[q]);
		const uint8_t *op = nullptr; i32 L = 0;
		if (gap_ops(a, x.i, x.ftype, x.f, op, L) && op) n += proj_wave(a, x, op, L, cnt);
	}
	for (int d = 32; d; d >>= 1) n += __shfl_xor(n, d);
	if (lane == 0 && n) atomicAdd(cnt + PJ_GAPCOLS, (unsigned long long)n);
}

// acc: the array at the range's first position, n positions -> text (16-byte aligned staging)
__global__ void __launch_bounds__(256) k_proj_text(const u32 *acc, i64 n, uint8_t *text)
{
	const unsigned long long tab = 0x3F2D4E544743416Eull;      // "nACGTN-?" by the word's low three bits: word 0 is 'n', a painted word carries a code 1..6
	const i64 j = ((i64)blockIdx.x * 256 + threadIdx.x) * 16;
	if (j >= n) return;
	if (j + 16 <= n) {
		u32 w[16];
		if ((((uintptr_t)(acc + j)) & 15u) == 0) { for (int q = 0; q < 4; q++) { const uint4 v = ((const uint4 *)(acc + j))[q]; w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w; } }
		else for (int q = 0; q < 16; q++) w[q] = acc[j + q];
		u32 o[4];
		for (int q = 0; q < 4; q++) { u32 r = 0; for (int e = 0; e < 4; e++) r |= (u32)((tab >> (8 * (w[4 * q + e] & 7u))) & 0xFFull) << (8 * e); o[q] = r; }
		*(uint4 *)(text + j) = make_uint4(o[0], o[1], o[2], o[3]);
	} else for (i64 q = j; q < n; q++) text[q] = (uint8_t)((tab >> (8 * (acc[q] & 7u))) & 0xFFull);
}

// src[0 .. n) into acc[0 .. n), the maximum stays; a wave instruction's atomics lie side by side
__global__ void __launch_bounds__(256) k_proj_merge(u32 *acc, i64 n, const u32 *src)
{
	const i64 base = (i64)blockIdx.x * 1024 + threadIdx.x;
	for (int q = 0; q < 4; q++) { const i64 i = base + 256 * q; if (i < n) { const u32 v = src[i]; if (v) atomicMax(acc + i, v); } }
}

// the launches of one contig; an error from here on leaves words nobody vouches for
static int proj_paint(gsa_ctx *c, const ProjIn &a, i64 span, i64 *hdr)
{
	hipStream_t st = c->stream;
	const i64 nwg = (a.W + 255) / 256;
	i64 *pre = c->d_ppre.as<i64>(), *wg = c->d_pwg.as<i64>();
	unsigned long long *cnt = (unsigned long long *)(wg + nwg);
	GSA_CHECK(c, hipMemsetAsync(cnt, 0, PJ_NCNT * sizeof(unsigned long long), st));
	hipLaunchKernelGGL(k_proj_prefix, dim3((unsigned)nwg), dim3(256), 0, st, a, pre, wg);
	GSA_CHECK(c, hipGetLastError());
	hipLaunchKernelGGL(k_wg_total<>, dim3(1), dim3(256), 0, st, nwg, wg, pre + a.W);
	GSA_CHECK(c, hipGetLastError());
	hipLaunchKernelGGL(k_proj_add, dim3((unsigned)nwg), dim3(256), 0, st, a.W, pre, (const i64 *)wg);
	GSA_CHECK(c, hipGetLastError());
	// (the run records' columns are at most the blocks' spans, which the host knows: no read-back sizes this grid)
	hipLaunchKernelGGL(k_proj_runs, dim3(grid_for((size_t)span, PROJ_TILE)), dim3(256), 0, st, a, (const i64 *)pre, cnt);
	GSA_CHECK(c, hipGetLastError());
	hipLaunchKernelGGL(k_proj_gaps, dim3((unsigned)nwg), dim3(256), 0, st, a, cnt);
	GSA_CHECK(c, hipGetLastError());
	GSA_CHECK(c, hipMemcpyAsync(hdr, pre + a.W, sizeof(i64), hipMemcpyDeviceToHost, st));
	GSA_CHECK(c, hipMemcpyAsync(hdr + 1, cnt, PJ_NCNT * sizeof(i64), hipMemcpyDeviceToHost, st));
	GSA_CHECK(c, hipStreamSynchronize(st));
	if (hdr[1 + PJ_NOJOB]) return gsa_fail(c, GSA_ERR_STATE, "internal: gsa_project met " + std::to_string((long long)hdr[1 + PJ_NOJOB]) + " DP record(s) without a DP job");
	if (hdr[1 + PJ_OUT]) return gsa_fail(c, GSA_ERR_STATE, "internal: gsa_project met " + std::to_string((long long)hdr[1 + PJ_OUT]) + " column(s) outside their record or sequence");
	return GSA_OK;
}

int project_blocks(gsa_ctx *c, i32 k, gsa_proj_stat *out)
{
	ProjAcc *pa = c->proj;
	if (pa->dirty.load()) return gsa_fail(c, GSA_ERR_STATE, "gsa_project: a failed pass left the accumulator dirty (gsa_proj_clear first)");
	const ResultRange rr = result_range(c, k);
	const size_t nb = rr.nb;
	if (nb == 0 || c->n_frags <= 0) return GSA_OK;
	if (!c->result_pinned) return gsa_fail(c, GSA_ERR_STATE, "gsa_project: the context holds no finished (stage 8) result");
	if (!pin_ensure<i64>(c, c->p_phdr, 1 + PJ_NCNT)) return GSA_ERR_NOMEM;
	// the painted blocks: duplicates too unless the accumulator was opened without them
	i32 nt = 0; i64 W = 0, span = 0;
	auto keep = [&](const gsa_block &bl) { return bl.bdup == 0 || !(c->proj_flags & GSA_PROJ_NO_DUP); };
	auto extra = [&](const gsa_block &bl, ProjBlk &v, const gsa_frag &, const gsa_frag &) {
		v.key = (bl.bdup == 0 ? 0x80000000u : 0u) | ((u32)std::min<i64>(std::max<i64>(bl.score, 0), (1 << 28) - 1) << 3);
		span += v.end - v.start;
		return (int)GSA_OK;
	};
	if (const int rc = span_build<ProjBlk>(c, rr, "gsa_project", c->p_pblk, 0, keep, extra, nt, W)) return rc;
	if (nt == 0) return GSA_OK;
	const i64 nwg = (W + 255) / 256;
	ENS(ProjBlk, d_pblk, (size_t)nt); ENS(i64, d_ppre, (size_t)W + 1); ENS(i64, d_pwg, (size_t)nwg + PJ_NCNT);      // sums | counters
	GSA_CHECK(c, hipMemcpyAsync(c->d_pblk.p, c->p_pblk.p, (size_t)nt * sizeof(ProjBlk), hipMemcpyHostToDevice, c->stream));
	ProjIn a;
	gap_in_fill(c, a);
	a.blk = c->d_pblk.as<ProjBlk>(); a.nb = nt; a.W = W; a.G = c->G; a.acc = pa->words;
	a.qtot = c->bnd.n ? c->b_off[(size_t)c->bnd.n] : c->qlen;
	i64 *hdr = c->p_phdr.as<i64>();
	if (const int rc = proj_paint(c, a, span, hdr)) { pa->dirty.store(1); return rc; }
	if (out) { out->n_blocks = nt; out->n_cols = hdr[0] + hdr[1 + PJ_GAPCOLS]; }
	return GSA_OK;
}

int proj_open(gsa_ctx *c, gsa_ctx *share, u32 flags)
{
	if (flags & ~(u32)GSA_PROJ_NO_DUP) return gsa_fail(c, GSA_ERR_ARG, "gsa_proj_open: unknown flags");
	if (c->proj) return gsa_fail(c, GSA_ERR_STATE, "gsa_proj_open: the context holds an accumulator already");
	if (share) {
		if (!share->proj) return gsa_fail(c, GSA_ERR_ARG, "gsa_proj_open: the context to share with holds no accumulator");
		if (share->proj->device != c->device || share->proj->G != c->G) return gsa_fail(c, GSA_ERR_ARG, "gsa_proj_open: the accumulator to share lies on another device (merge its words with gsa_proj_merge)");
		share->proj->refs.fetch_add(1);
		c->proj = share->proj; c->proj_flags = flags;
		return GSA_OK;
	}
	if (c->G <= 0) return gsa_fail(c, GSA_ERR_STATE, "gsa_proj_open: the context holds no reference");
	GSA_CHECK(c, hipSetDevice(c->device));
	void *p = nullptr;
	if (hipMalloc(&p, (size_t)c->G * sizeof(u32)) != hipSuccess) { (void)hipGetLastError(); return gsa_fail(c, GSA_ERR_NOMEM, "gsa_proj_open: hipMalloc of " + std::to_string((long long)c->G * 4) + " bytes"); }
	hipError_t e = hipMemsetAsync(p, 0, (size_t)c->G * sizeof(u32), c->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
	if (e != hipSuccess) { hipFree(p); return gsa_fail(c, GSA_ERR_HIP, std::string("gsa_proj_open: ") + hipGetErrorString(e)); }
	ProjAcc *pa = new ProjAcc(); pa->words = (u32 *)p; pa->G = c->G; pa->device = c->device;
	c->proj = pa; c->proj_flags = flags;
	return GSA_OK;
}

int proj_release(gsa_ctx *c)
{
	ProjAcc *pa = c->proj;
	if (!pa) return GSA_OK;
	hipSetDevice(c->device);
	ctx_quiesce(c);      // (nothing of this context paints any more; the other holders let go behind their own streams)
	c->proj = nullptr; c->proj_flags = 0;
	if (pa->refs.fetch_sub(1) == 1) { hipFree(pa->words); delete pa; }
	return GSA_OK;
}

int proj_clear(gsa_ctx *c)
{
	ProjAcc *pa = c->proj;
	GSA_CHECK(c, hipSetDevice(c->device));
	GSA_CHECK(c, hipMemsetAsync(pa->words, 0, (size_t)pa->G * sizeof(u32), c->stream));
	GSA_CHECK(c, hipStreamSynchronize(c->stream));
	pa->dirty.store(0);
	return GSA_OK;
}

int proj_fetch(gsa_ctx *c, i64 p0, i64 n, char *text, u32 *words)
{
	ProjAcc *pa = c->proj;
	if (pa->dirty.load()) return gsa_fail(c, GSA_ERR_STATE, "gsa_proj_fetch: a failed pass left the accumulator dirty (gsa_proj_clear first)");
	GSA_CHECK(c, hipSetDevice(c->device));
	hipStream_t st = c->stream;
	for (i64 off = 0; off < n; off += PROJ_CHUNK) {
		const i64 m = std::min<i64>(PROJ_CHUNK, n - off);
		const u32 *src = pa->words + p0 + off;
		if (!pin_ensure<u32>(c, c->p_pstage, (size_t)m)) return GSA_ERR_NOMEM;
		if (words) {
			GSA_CHECK(c, hipMemcpyAsync(c->p_pstage.p, src, (size_t)m * sizeof(u32), hipMemcpyDeviceToHost, st));
			GSA_CHECK(c, hipStreamSynchronize(st));
			memcpy(words + off, c->p_pstage.p, (size_t)m * sizeof(u32));
		}
		if (text) {
			ENS(u32, d_pstage, (size_t)m);
			hipLaunchKernelGGL(k_proj_text, dim3(grid_for((size_t)(m + 15) / 16, 256)), dim3(256), 0, st, src, m, c->d_pstage.as<uint8_t>());
			GSA_CHECK(c, hipGetLastError());
			GSA_CHECK(c, hipMemcpyAsync(c->p_pstage.p, c->d_pstage.p, (size_t)m, hipMemcpyDeviceToHost, st));
			GSA_CHECK(c, hipStreamSynchronize(st));
			memcpy(text + off, c->p_pstage.p, (size_t)m);
		}
	}
	return GSA_OK;
}

int proj_merge(gsa_ctx *c, i64 p0, i64 n, const u32 *words)
{
	ProjAcc *pa = c->proj;
	GSA_CHECK(c, hipSetDevice(c->device));
	hipStream_t st = c->stream;
	for (i64 off = 0; off < n; off += PROJ_CHUNK) {
		const i64 m = std::min<i64>(PROJ_CHUNK, n - off);
		if (!pin_ensure<u32>(c, c->p_pstage, (size_t)m)) return GSA_ERR_NOMEM;
		ENS(u32, d_pstage, (size_t)m);
		memcpy(c->p_pstage.p, words + off, (size_t)m * sizeof(u32));
		GSA_CHECK(c, hipMemcpyAsync(c->d_pstage.p, c->p_pstage.p, (size_t)m * sizeof(u32), hipMemcpyHostToDevice, st));
		hipLaunchKernelGGL(k_proj_merge, dim3(grid_for((size_t)(m + 3) / 4, 256)), dim3(256), 0, st, pa->words + p0 + off, m, (const u32 *)c->d_pstage.as<u32>());
		GSA_CHECK(c, hipGetLastError());
		GSA_CHECK(c, hipStreamSynchronize(st));      // (the staging buffers are filled again in the next round)
	}
	return GSA_OK;
}
