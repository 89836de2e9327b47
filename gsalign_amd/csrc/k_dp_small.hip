// gsalign_amd/csrc/k_dp_small.hip -- gap-closing DP (a13), the size classes below the striped kernel (n <= 64 and
// m + n - 1 <= 128: the bulk of the jobs, median 11 x 11).  Cell recurrence and traceback automaton: gsa_dp.h; how the
// jobs are sorted into classes: k_dp.hip.
//  * k_dp_small  one wavefront per alignment, lane t owns target column t.  The (u,v,x,y) state
//    lives in REGISTERS; the left neighbour and the reference base travel one lane
//    up per anti-diagonal with DPP wave shifts (systolic array); direction bytes
//    and the traceback stay in LDS.  No barrier, no global traffic but the result.
//  * k_dp_lane   one LANE per alignment of at most `dp_lane` cells; see the comment at the kernel.
#include "gsa_ctx.h"
#include "gsa_dp.h"
#include "gsa_gap.h"

#define SMALL_WAVES 4

__global__ void __launch_bounds__(64 * SMALL_WAVES) k_dp_small(i32 n_jobs, const i32 *__restrict__ order, const uint8_t *__restrict__ pool1, const i64 *__restrict__ off1,
                                                                const i32 *__restrict__ len1, const uint8_t *__restrict__ pool2, const i64 *__restrict__ off2,
                                                                const i32 *__restrict__ len2, uint8_t *ops, const i64 *__restrict__ ops_off, i32 *ops_len,
                                                                const i32 *__restrict__ jfrag, gsa_frag *frag)
{
	// direction flags as NIBBLES, two anti-diagonals per byte (only bits 0-1 and 3-4 of ksw2's flag byte are ever set): half
	// the LDS per alignment -- LDS is what limits how many of these waves a CU holds -- and half the LDS stores
	__shared__ uint8_t s_dir[SMALL_WAVES][(SMALL_ROWS / 2) * 64];
	__shared__ uint8_t s_rev[SMALL_WAVES][SMALL_ROWS + 64];
	__shared__ int s_n[SMALL_WAVES];
	const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const i32 slot = blockIdx.x * SMALL_WAVES + w;
	if (slot >= n_jobs) return;
	// (the job and its two lengths are the same in all lanes: said so, they live in scalar registers, the loop over the anti-diagonals is
	//  uniform and the reference base that enters at lane 0 is READ from its lane (v_readlane) instead of fetched through the LDS crossbar
	//  (ds_bpermute): that fetch sat in front of every diagonal's dependent chain)
	const i32 job = __builtin_amdgcn_readfirstlane(order[slot]);
	const int m = __builtin_amdgcn_readfirstlane(len1[job]), n = __builtin_amdgcn_readfirstlane(len2[job]);
	const uint8_t *s1 = pool1 + off1[job], *s2 = pool2 + off2[job];
	uint8_t *dir = s_dir[w], *rev = s_rev[w];
	const int cq = lane < n ? gsa_nt4(s2[lane]) : 4;
	// reference base for lane t at diagonal r is s1[r - t]: it enters at lane 0 and moves one lane up per diagonal
	const int c1a = lane < m ? gsa_nt4(s1[lane]) : 4, c1b = lane + 64 < m ? gsa_nt4(s1[lane + 64]) : 4;
	int u = lane ? 2 : 0, v = 0, x = 0, y = 0, wref = 4, dacc = 0;
	const int nr = m + n - 1;
	for (int r = 0; r < nr; r++) {
		const int inb = r < m ? (r < 64 ? __builtin_amdgcn_readlane(c1a, r) : __builtin_amdgcn_readlane(c1b, r - 64)) : 4;      // s1[r] broadcast
		wref = wave_shr1(wref, inb);
		const int xt1 = wave_shr1(x, 0), vt1 = wave_shr1(v, r ? 2 : 0);                     // (r-1,t-1); boundary for t = 0 (:157-164)
		const int jj = r - lane;
		int d = 0;
		if (lane < n && jj >= 0 && jj < m) {
			int un, vn, xn, yn;
			d = dp_cell(xt1, vt1, u, y, cq, wref, un, vn, xn, yn);
			u = un; v = vn; x = xn; y = yn;
		}
		const int nib = (d & 3) | ((d & 0x18) >> 1);
		// (every lane stores, cells outside the matrix are never read)
		if (r & 1) dir[(r >> 1) * 64 + lane] = (uint8_t)(dacc | (nib << 4)); else dacc = nib;
	}
	if (nr & 1) dir[(nr >> 1) * 64 + lane] = (uint8_t)dacc;
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
	if (lane == 0) {
		int i = n - 1, j = m - 1, state = 0, k = 0;
		while (i >= 0 && j >= 0) {
			const u32 nb = ((u32)dir[((i + j) >> 1) * 64 + i] >> (((i + j) & 1) << 2)) & 15u;
			const u32 tmp = (nb & 3u) | ((nb & 0xCu) << 1);
			state = dp_bt_next(state, tmp);
			const int isM = state == 0 ? 1 : 0, isD = (state == 1 || state == 3) ? 1 : 0;
			rev[k++] = (uint8_t)(isM ? 'M' : (isD ? 'D' : 'I'));
			i -= isM | isD; j -= isM | (1 - isD);
		}
		for (; i >= 0; --i) rev[k++] = 'D';
		for (; j >= 0; --j) rev[k++] = 'I';
		s_n[w] = k;
	}
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
	const int nops = s_n[w];
	uint8_t *op = ops + ops_off[job];
	for (int p = lane; p < nops; p += 64) op[p] = rev[nops - 1 - p];
	if (lane == 0) { ops_len[job] = nops; if (frag) frag[jfrag[job]].aln_len = nops; }      // (the job's record is final with this)
}

// ---------------------------------------------------------------------------
// k_dp_lane (round 3): ONE LANE PER ALIGNMENT for the smallest jobs of the class below the striped kernel (n <= 64, m + n - 1 <= 128: 360 000 jobs and
// 104 M cells of a human-sized contig -- 7 % of the cells, but k_dp_small and round 2's four-per-wavefront k_dp_tiny spent 4.7 VALU instructions per cell on them,
// ten times the striped kernel: a systolic wave has 23 of 64 lanes busy on the median job, moves three values by DPP per step and
// walks back on one lane).  A lane needs no neighbour: cell (i, j) takes x, v from the cell on its left (registers) and u, y from
// the cell above (one 16-bit LDS entry per column, with the query base's code), row by row -- the same recurrence in another
// order (dp_cell is order-free: gsa_dp.h), so every lane is busy on every instruction.  What has to be managed is balance: a
// wavefront runs as long as its largest job.  A workgroup takes a tile of 512 jobs, counting-sorts it by cells (128 logarithmic
// bins in LDS) and its four waves draw batches of 64 size-neighbours, largest first.  Direction nibbles go to a per-wave arena in
// global memory (L2-resident: eight cells per dword, dword k of lane l at [k][l] -- coalesced), the traceback automaton reads them
// back, the reversed op string is staged in the LDS of the (dead) column entries.
// ---------------------------------------------------------------------------
#define LANE_TILE 512
#define LANE_BINS 128
#define LANE_KMAX 576           // direction dwords of one job at most: m * ceil(n / 8) with n <= 64, m + n - 1 <= 128 (n = 57, m = 72)
#ifndef LANE_WGS
#define LANE_WGS 1024           // persistent workgroups (four per CU: 38 KB of LDS each)
#endif
#define LANE_LDS_WAVE 8448      // 64 columns x 64 lanes x 2 bytes (forward)  |  (128 + 2) op bytes x 64 lanes (traceback)
__device__ __forceinline__ u32 lane_bin(u32 cells)      // floor(8 log2 cells): 1 <= cells < 8192 -> 0 .. 103
{
	const int msb = 31 - __clz((int)cells);
	const u32 frac = msb >= 3 ? (cells >> (msb - 3)) & 7u : (cells << (3 - msb)) & 7u;
	return ((u32)msb << 3) | frac;
}

__global__ void __launch_bounds__(256) k_dp_lane(i32 n_jobs, const i32 *__restrict__ order,
                                                  const uint8_t *__restrict__ pool1, const i64 *__restrict__ off1, const i32 *__restrict__ len1,
                                                  const uint8_t *__restrict__ pool2, const i64 *__restrict__ off2, const i32 *__restrict__ len2,
                                                  uint8_t *ops, const i64 *__restrict__ ops_off, i32 *ops_len, const i32 *__restrict__ jfrag, gsa_frag *frag, u32 *arena_all, u32 kstride)
{
	__shared__ u32 s_hist[LANE_BINS];
	__shared__ i32 s_sorted[LANE_TILE];
	__shared__ int s_next;
	__shared__ __attribute__((aligned(16))) uint8_t s_work[4][LANE_LDS_WAVE];
	const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
	u32 *arena = arena_all + ((size_t)blockIdx.x * 4 + w) * 64 * kstride + lane;      // dword k of my job: arena[k * 64]; kstride = the most dwords a job of this launch's class can need
	uint16_t *col = (uint16_t *)s_work[w] + lane;                                         // column i of my job: col[i * 64]
	uint8_t *revb = s_work[w] + lane;                                                     // reversed op k of my job: revb[k * 64]
	for (i64 t0 = (i64)blockIdx.x * LANE_TILE; t0 < n_jobs; t0 += (i64)gridDim.x * LANE_TILE) {
		// ---- the tile's jobs, largest first (counting sort by cells) ----
		if (tid < LANE_BINS) s_hist[tid] = 0;
		if (tid == 0) s_next = 0;
		__syncthreads();
		i32 jb[LANE_TILE / 256]; u32 key[LANE_TILE / 256], rk[LANE_TILE / 256];
#pragma unroll
		for (int k = 0; k < LANE_TILE / 256; k++) {
			const i64 idx = t0 + k * 256 + tid;
			jb[k] = -1; key[k] = 0; rk[k] = 0;
			if (idx < n_jobs) {
				const i32 job = order[idx];
				jb[k] = job; key[k] = lane_bin((u32)len1[job] * (u32)len2[job]); rk[k] = atomicAdd(&s_hist[key[k]], 1u);
			}
		}
		__syncthreads();
		if (tid < 64) {      // exclusive prefix over the bins in descending order (two bins per lane)
			const u32 a = s_hist[LANE_BINS - 1 - 2 * lane], b = s_hist[LANE_BINS - 2 - 2 * lane];
			u32 inc = a + b;
			for (int o = 1; o < 64; o <<= 1) { const u32 t = __shfl_up(inc, o); if (lane >= o) inc += t; }
			const u32 ex = inc - (a + b);
			s_hist[LANE_BINS - 1 - 2 * lane] = ex; s_hist[LANE_BINS - 2 - 2 * lane] = ex + a;
		}
		__syncthreads();
#pragma unroll
		for (int k = 0; k < LANE_TILE / 256; k++) if (jb[k] >= 0) s_sorted[s_hist[key[k]] + rk[k]] = jb[k];
		__syncthreads();
		const int nt = (int)(n_jobs - t0 < LANE_TILE ? n_jobs - t0 : LANE_TILE), nb = (nt + 63) >> 6;
		for (;;) {
			int b = 0;
			if (lane == 0) b = atomicAdd(&s_next, 1);
			b = __builtin_amdgcn_readfirstlane(b);
			if (b >= nb) break;
			const int p = b * 64 + lane;
			const bool have = p < nt;
			const i32 job = have ? s_sorted[p] : 0;
			const int m = have ? len1[job] : 0, n = have ? len2[job] : 0;
			const uint8_t *s1 = pool1 + off1[job], *s2 = pool2 + off2[job];
			const int nw = (n + 7) >> 3;
			// column entries: u (5 bits) | y << 5 (5 bits) | 4 * code of the query base << 10; before row 0: u = 2 (0 in column 0), y = 0
			int nmax = n;
			for (int o = 32; o; o >>= 1) { const int t = __shfl_xor(nmax, o); nmax = t > nmax ? t : nmax; }
			for (int i = 0; i < nmax; i++) if (i < n) col[i * 64] = (uint16_t)((i ? 2 : 0) | (gsa_nt4(s2[i]) << 12));
			// ---- forward: row j = reference base, columns in GROUPS OF EIGHT (one direction dword; its eight entries are read together,
			//      the cells follow one another through x, v in registers, the loop control is paid once per group) ----
			bool act = have && m > 0 && n > 0;
			int g = 0, j = 0, x = 0, v = 0, kk = 0;
			// z = score + q + e of (query code a, row base b) as a nibble table over a: 7 match, 5 mismatch, 6 when either is N
			auto row_table = [](int b) -> u32 { return b == 4 ? 0x66666u : 0x65555u + (2u << (4 * b)); };
			u32 tbl = row_table(act ? gsa_nt4(s1[0]) : 4);
			uint8_t raw_next = (act && m > 1) ? s1[1] : (uint8_t)'N';      // (the next row's base: loaded a row ahead, decoded when the row starts)
			while (__any(act)) {
				if (act) {
					uint16_t *cg = col + g * 8 * 64;
					u32 e[8];
#pragma unroll
					for (int k = 0; k < 8; k++) e[k] = cg[k * 64];
					u32 acc = 0;
					const int left = n - g * 8;                            // valid columns of this group (>= 1; 8 or more: all)
#pragma unroll
					for (int k = 0; k < 8; k++) {
						if (k < left) {
							const int u = (int)(e[k] & 31u), y = (int)((e[k] >> 5) & 31u);
							const u32 c4 = e[k] >> 10;
							int z = (int)((tbl >> c4) & 15u);
							int a = x + v, b = y + u;
							int d = a > z ? 1 : 0; z = z > a ? z : a;
							if (b > z) d = 2;
							z = z > b ? z : b;
							z = z < 7 ? z : 7;
							const int un = z - v, vn = z - u;
							z -= 2; a -= z; b -= z;
							if (a > 0) d |= 0x08; else a = 0;
							if (b > 0) d |= 0x10; else b = 0;
							cg[k * 64] = (uint16_t)((u32)un | ((u32)b << 5) | (c4 << 10));
							x = a; v = vn;
							acc |= (u32)((d & 3) | ((d & 0x18) >> 1)) << (4 * k);
						}
					}
					arena[(size_t)kk * 64] = acc; kk++;
					g++;
					if (g == nw) {
						g = 0; j++; x = 0; v = 2;      // (left boundary of row j > 0: x = 0, v = 2; ksw2_alignment.cpp:157-164)
						if (j >= m) act = false;
						else { tbl = row_table(gsa_nt4(raw_next)); raw_next = j + 1 < m ? s1[j + 1] : (uint8_t)'N'; }
					}
				}
			}
			// ---- traceback (dp_bt_next, gsa_dp.h), one lane per job; the reversed ops go where the column entries were ----
			int ti = n - 1, tj = m - 1, state = 0, k = 0;
			bool tb = have && ti >= 0 && tj >= 0;
			while (__any(tb)) {
				if (tb) {
					const u32 wd = arena[(size_t)(tj * nw + (ti >> 3)) * 64];
					const u32 nbv = (wd >> ((ti & 7) << 2)) & 15u;
					const u32 tmp = (nbv & 3u) | ((nbv & 0xCu) << 1);
					state = dp_bt_next(state, tmp);
					const int isM = state == 0 ? 1 : 0, isD = (state == 1 || state == 3) ? 1 : 0;
					revb[k * 64] = (uint8_t)(isM ? 'M' : (isD ? 'D' : 'I'));
					k++;
					ti -= isM | isD; tj -= isM | (1 - isD);
					tb = ti >= 0 && tj >= 0;
				}
			}
			if (have) {
				for (; ti >= 0; --ti) { revb[k * 64] = 'D'; k++; }
				for (; tj >= 0; --tj) { revb[k * 64] = 'I'; k++; }
				uint8_t *op = ops + ops_off[job];
				for (int q = 0; q < k; q++) op[q] = revb[(k - 1 - q) * 64];
				ops_len[job] = k;
				if (frag) frag[jfrag[job]].aln_len = k;      // (the job's record is final with this)
			}
		}
		__syncthreads();      // (the next tile reuses the bins and the sorted list)
	}
}

// Both classes of a job list, on a second stream beside the striped kernel: the one-per-lane jobs on stream_aux[1], the one-per-wavefront
// jobs beside them on the caller's stream `st` (on stream_aux[1] when there is nothing per lane) and joined into stream_aux[1].  Event
// ev[12] marks the end of both; the caller decides what waits for it.
// (Not a stream of its own for k_dp_small: the runtime maps streams onto four hardware queues, a fifth stream shares one -- with the
//  striped kernel, if it is unlucky)
int launch_small_dp(gsa_ctx *c, hipStream_t st, i32 nlane, const i32 *order_lane, i32 nsmall, const i32 *order_small, const uint8_t *pool1, const i64 *off1, const i32 *len1,
                    const uint8_t *pool2, const i64 *off2, const i32 *len2, uint8_t *ops, const i64 *ops_off, i32 *ops_len, const i32 *jfrag, gsa_frag *frag)
{
	hipStream_t sl = c->stream_aux[1];
	GSA_CHECK(c, hipEventRecord(c->ev[10], st));
	GSA_CHECK(c, hipStreamWaitEvent(sl, c->ev[10], 0));
	if (nlane > 0) {
		const i64 tiles = ((i64)nlane + LANE_TILE - 1) / LANE_TILE;
		const unsigned nwg = (unsigned)(tiles < LANE_WGS ? tiles : LANE_WGS);
		// direction dwords of one job at most: m * ceil(n / 8) over the shapes of the class (n <= 64, m + n - 1 <= 128, m * n <= dp_lane cells): 128 for
		// the default 512 cells, LANE_KMAX = 576 without a cell limit -- the arena was always sized for the latter: 604 MB per context instead of 134
		const int dp_lane = c->opt.dp_lane;
		u32 kstride = 1;
		for (int nn = 1; nn <= 64; nn++) { int mm = 128 - nn + 1; if (dp_lane / nn < mm) mm = dp_lane / nn; if (mm < 1) continue; const u32 kd = (u32)mm * (u32)((nn + 7) / 8); if (kd > kstride) kstride = kd; }
		if (kstride > LANE_KMAX) kstride = LANE_KMAX;
		u32 *arena = dev_ensure<u32>(c, c->d_dp_arena, (size_t)nwg * 4 * 64 * kstride);
		if (!arena) return GSA_ERR_NOMEM;
		hipLaunchKernelGGL(k_dp_lane, dim3(nwg), dim3(256), 0, sl, nlane, order_lane, pool1, off1, len1, pool2, off2, len2, ops, ops_off, ops_len, jfrag, frag, arena, kstride);
	}
	if (nsmall > 0) {
		hipStream_t s2 = nlane > 0 ? st : sl;
		const unsigned nb = (unsigned)((nsmall + SMALL_WAVES - 1) / SMALL_WAVES);
		hipLaunchKernelGGL(k_dp_small, dim3(nb), dim3(64 * SMALL_WAVES), 0, s2, nsmall, order_small, pool1, off1, len1, pool2, off2, len2, ops, ops_off, ops_len, jfrag, frag);
		if (nlane > 0) { GSA_CHECK(c, hipEventRecord(c->ev[18], s2)); GSA_CHECK(c, hipStreamWaitEvent(sl, c->ev[18], 0)); }
	}
	GSA_CHECK(c, hipGetLastError());
	GSA_CHECK(c, hipEventRecord(c->ev[12], sl));
	return GSA_OK;
}
