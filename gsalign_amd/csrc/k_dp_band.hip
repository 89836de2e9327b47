// gsalign_amd/csrc/k_dp_band.hip -- gap-closing DP (a13), the band class: near-diagonal jobs of a striped batch, evaluated inside a window of
// DP_BAND_DIAGS diagonals, each with an exactness certificate; a job that fails it keeps nothing and runs in k_dp_stripe as before.  Cell in absolute
// scores, layout, certificate and traceback automaton: gsa_dp.h; who calls this: launch_stripes (k_dp_stripe.hip).
#include <algorithm>
#include "gsa_ctx.h"
#include "gsa_dp.h"

// ---------------------------------------------------------------------------
// k_dp_band: ONE WAVEFRONT PER TWO JOBS, X in the low and Y in the high 16-bit halves of every register, a step per anti-diagonal.
// Step s is anti-diagonal r = i + j = s - 2 (the two steps in front compute the boundary row and column).  Lane l owns the diagonals
// d = base + 2l and d + 1 of its job (base even): a cell's diagonal has the parity of its anti-diagonal, so on even steps every lane
// computes its even diagonal, on odd steps its odd one -- every lane is busy on every step, and a job takes m + n + 1 steps.
// A cell needs H(i-1,j-1) (its own diagonal, two steps ago: a register), E(i,j) from (i-1,j) (diagonal d - 1, one step ago) and F(i,j) from
// (i,j-1) (diagonal d + 1, one step ago): on an even step E comes from lane l - 1 (one DPP shift up) and F is the lane's own; on an odd
// step E is the lane's own and F comes from lane l + 1 (one DPP shift down).  The shifts fill the window's two ends with DP_BAND_NEG.
// Both jobs' base codes arrive as ONE dword per position (k_dp_band_prep): Q[p] holds s2X[p + baseX/2 - 1] | s2Y[p + baseY/2 - 1] << 16,
// R[p] the reference sides at p - 65 - base/2, so that on step s lane l reads Q[s/2 + l (+1 on odd steps)] and R[s/2 - l + 64] whatever the
// jobs' windows are: four positions of each per eight steps, fetched one chunk ahead, no LDS.  Positions outside a fragment hold N.
// Direction nibbles (ta | tb << 1 | fa << 2 | fb << 3, as the striped kernel packs them) go to HBM: per job and eight steps one dword per lane.
// The cells of the first steps that lie in front of row 0 or column 0 are overwritten with the boundary values (GUARD chunks: H = -(2 + s) on
// step s, 0 in the corner); cells behind a fragment's end compute on N and reach nothing.
// After the last step the lane of diagonal n - m holds the band score.  If it beats dp_band_ub, the same wave walks back -- an M run per
// look: lane e fetches the dword of its column eight-step block e blocks back, a ballot gives the run's length -- writes the job's ops
// and tags it certified; otherwise it writes nothing.
// The window is a superset of the band the certificate speaks of ([lo, hi] of gsa_dp.h): where the certificate holds, every optimal path and every
// prefix that ties one lies inside [lo, hi], so window and band give the same flags along the path; where it fails, the job is not kept either way;
// and whether it holds does not depend on the window: it holds exactly when the full-matrix optimum exceeds UB.
// ---------------------------------------------------------------------------
typedef short v2i16 __attribute__((ext_vector_type(2)));
typedef unsigned short v2u16b __attribute__((ext_vector_type(2)));
#define BI(X) __builtin_bit_cast(v2i16, (u32)(X))
#define BU(X) __builtin_bit_cast(u32, (X))
__device__ __forceinline__ u32 bk_add(u32 a, u32 b) { return BU(BI(a) + BI(b)); }
__device__ __forceinline__ u32 bk_sub(u32 a, u32 b) { return BU(BI(a) - BI(b)); }
__device__ __forceinline__ u32 bk_max(u32 a, u32 b) { return BU(__builtin_elementwise_max(BI(a), BI(b))); }
__device__ __forceinline__ u32 bk_min(u32 a, u32 b) { return BU(__builtin_elementwise_min(BI(a), BI(b))); }
__device__ __forceinline__ u32 bk_mad(u32 a, u32 b, u32 c) { return BU(__builtin_bit_cast(v2u16b, a) * __builtin_bit_cast(v2u16b, b) + __builtin_bit_cast(v2u16b, c)); }
__device__ __forceinline__ u32 bk_sar15(u32 a) { return BU(BI(a) >> (v2i16)(15)); }
__device__ __forceinline__ u32 bk_shr2(u32 a) { return BU(__builtin_bit_cast(v2u16b, a) >> (v2u16b)(2)); }
#define BAND_OPAQUE(X) asm volatile("" : "+v"(X))
#define BAND_NEG2 (((u32)(DP_BAND_NEG & 0xffff)) * 0x10001u)

struct __attribute__((packed, aligned(4))) BandQuad { u32 a, b, c, d; };

// steps of a pair (a multiple of eight) and positions of each of its two code strings
__host__ __device__ static inline int band_steps8(const BandJob &x, const BandJob &y) { const int sx = x.m + x.n, sy = y.job >= 0 ? y.m + y.n : 0; return ((sx > sy ? sx : sy) + 1 + 7) & ~7; }
__host__ __device__ static inline int band_seq_len(int steps8) { return steps8 / 2 + 72; }

// the pairs' code strings: s2 sides 0-3 / N 4, s1 sides 0-3 / N 8 (the XOR of a column's two codes is 0: match, 1-3: mismatch, >= 4: an N)
__global__ void __launch_bounds__(256) k_dp_band_prep(const BandJob *__restrict__ jobs, const uint8_t *__restrict__ pool1, const i64 *__restrict__ off1, const uint8_t *__restrict__ pool2, const i64 *__restrict__ off2,
                                                      u32 *__restrict__ seq, u32 *__restrict__ hasn)
{
	const int p = blockIdx.x;
	const BandJob X = jobs[2 * p], Y = jobs[2 * p + 1];
	const int LQ = band_seq_len(band_steps8(X, Y));
	u32 *Q = seq + X.seqoff, *R = Q + LQ;
	const bool hy = Y.job >= 0;
	const uint8_t *s1x = pool1 + off1[X.job], *s2x = pool2 + off2[X.job];
	const uint8_t *s1y = hy ? pool1 + off1[Y.job] : s1x, *s2y = hy ? pool2 + off2[Y.job] : s2x;
	const int my = hy ? Y.m : 0, ny = hy ? Y.n : 0;
	int anyn = 0;
	for (int t = threadIdx.x; t < LQ; t += 256) {
		const int ix = t + X.base / 2 - 1, iy = t + Y.base / 2 - 1, jx = t - 65 - X.base / 2, jy = t - 65 - Y.base / 2;
		const u32 qx = (ix >= 0 && ix < X.n) ? (u32)gsa_nt4(s2x[ix]) : 4u, qy = (iy >= 0 && iy < ny) ? (u32)gsa_nt4(s2y[iy]) : 4u;
		u32 rx = (jx >= 0 && jx < X.m) ? (u32)gsa_nt4(s1x[jx]) : 4u, ry = (jy >= 0 && jy < my) ? (u32)gsa_nt4(s1y[jy]) : 4u;
		anyn |= ((ix >= 0 && ix < X.n && qx == 4) || (iy >= 0 && iy < ny && qy == 4) || (jx >= 0 && jx < X.m && rx == 4) || (jy >= 0 && jy < my && ry == 4)) ? 1 : 0;
		rx = rx == 4 ? 8u : rx; ry = ry == 4 ? 8u : ry;
		Q[t] = qx | (qy << 16); R[t] = rx | (ry << 16);
	}
	anyn = __syncthreads_or(anyn);
	if (threadIdx.x == 0) hasn[p] = (u32)anyn;
}

struct BandState {
	u32 h1e, h1o;      // H + 1 of the lane's last cell on its even / odd diagonal
	u32 ee, fe, eo, fo;      // E(i+1,j), F(i,j+1) out of those cells
	u32 acc, r0;      // direction nibbles of the last four steps (per half, oldest on top); those of the four before
	u32 iv, jv;      // GUARD: i, j of the current cell, both jobs
	u32 capx, capy;      // H + 1 of the two jobs' last cells
};

// Eight steps from s0 on.  q0-q4, r0-r3: the chunk's codes (q4: the first of the next chunk).  HASN: a fragment of the pair holds an N (score 0).
// GUARD: some lane's cell lies in front of row 0 / column 0.  CAP: a job's last cell is computed in this chunk.
template <bool HASN, bool GUARD, bool CAP>
__device__ __forceinline__ void band_chunk(BandState &S, int s0, const u32 (&q)[5], const u32 (&r)[4], u32 c1, u32 c2, u32 c4, u32 c16, u32 cm2,
                                           int sfx, int lfx, int sfy, int lfy)
{
#pragma unroll
	for (int k = 0; k < 8; k++) {
		const bool odd = k & 1;
		const u32 a = q[(k + 1) >> 1], b = r[k >> 1];
		const u32 ein = odd ? S.ee : (u32)wave_shr1((int)S.eo, (int)BAND_NEG2);
		const u32 fin = odd ? (u32)wave_shl1((int)S.fe, (int)BAND_NEG2) : S.fo;
		const u32 e = a ^ b, t = bk_min(e, c1);
		u32 hd = bk_mad(t, cm2, odd ? S.h1o : S.h1e);      // H(i-1,j-1) + 1 - 2 (mismatch)
		if (HASN) hd = bk_add(hd, bk_min(bk_shr2(e), c1));      // ... + 1 where a side is N
		const u32 d1 = bk_max(hd, ein), ta = bk_min(bk_sub(d1, hd), c1);
		const u32 h = bk_max(d1, fin), tb = bk_min(bk_sub(h, d1), c1);
		const u32 hq = bk_sub(h, c2);
		const u32 me = bk_max(ein, hq), mf = bk_max(fin, hq);
		const u32 fa = bk_min(bk_sub(me, hq), c1), fb = bk_min(bk_sub(mf, hq), c1);
		u32 en = bk_sub(me, c1), fn = bk_sub(mf, c1), h1 = bk_add(h, c1);
		S.acc = bk_mad(S.acc, c16, bk_mad(bk_mad(fb, c2, fa), c4, bk_mad(tb, c2, ta)));
		if (GUARD) {
			const int s = s0 + k;
			const u32 hb = (u32)((s == 0 ? 0 : -(2 + s)) & 0xffff) * 0x10001u;      // H of a boundary cell of this anti-diagonal
			const u32 neg = bk_sar15(S.iv | S.jv);
			h1 = (neg & bk_add(hb, c1)) | (~neg & h1);
			const u32 hb3 = bk_sub(hb, bk_add(c2, c1));
			en = (neg & hb3) | (~neg & en); fn = (neg & hb3) | (~neg & fn);
			if (odd) S.jv = bk_add(S.jv, c1); else S.iv = bk_add(S.iv, c1);
		}
		if (odd) { S.h1o = h1; S.eo = en; S.fo = fn; } else { S.h1e = h1; S.ee = en; S.fe = fn; }
		if (CAP) {
			if (s0 + k == sfx) S.capx = (u32)__builtin_amdgcn_readlane((int)h1, lfx);
			if (s0 + k == sfy) S.capy = (u32)__builtin_amdgcn_readlane((int)h1, lfy);
		}
		if (k == 3) S.r0 = S.acc;
	}
}

__device__ __forceinline__ u32 band_nib_shift(int t) { return (u32)(((t >> 2) << 4) + ((3 - (t & 3)) << 2)); }

// The walk back of one certified job, by the whole wave: ops and ops_len as the striped kernel writes them.
__device__ __forceinline__ void band_walk(const u32 *__restrict__ dirj, int m, int n, int base, uint8_t *rev, uint8_t *op, i32 *len_out, int lane)
{
	int i = n - 1, j = m - 1, state = 0, k = 0;
	while (i >= 0 && j >= 0) {
		i = __builtin_amdgcn_readfirstlane(i); j = __builtin_amdgcn_readfirstlane(j);
		state = __builtin_amdgcn_readfirstlane(state); k = __builtin_amdgcn_readfirstlane(k);
		const int s = i + j + 2, col = (i - j - base) >> 1, blk = s >> 3, t = s & 7;
		// lane e: the eight-step block e blocks back, in the current cell's column (the cells of its diagonal are the nibbles of t's parity)
		const int bb = blk - lane;
		const u32 w = bb >= 0 ? dirj[((size_t)bb << 6) + col] : 0xffffffffu;
		const u32 nb = ((u32)__builtin_amdgcn_readfirstlane((int)w) >> band_nib_shift(t)) & 15u;
		const u32 cur = ((nb & 2u) ? 2u : (nb & 1u)) | ((nb & 0xCu) << 1);      // back to ksw2's flag byte
		const int S = dp_bt_next(state, cur);
		state = S;
		if (S != 0) {
			if (lane == 0) rev[k] = (uint8_t)(S == 2 ? 'I' : 'D');
			k++;
			if (S == 2) j--; else i--;
			continue;
		}
		// an M: and the cells behind it on the diagonal while their direction is the diagonal too (state 0 stays 0)
		const int tp0 = lane == 0 ? t - 2 : 6 + (t & 1), ncand = lane == 0 ? (t >> 1) : 4;
		int cnt = 0; bool ok = true;
#pragma unroll
		for (int c4 = 0; c4 < 4; c4++) {
			const int tp = tp0 - 2 * c4;
			ok = ok && tp >= 0 && ((w >> band_nib_shift(tp & 7)) & 3u) == 0;
			cnt += ok ? 1 : 0;
		}
		const unsigned long long full = __ballot(cnt == ncand);
		int run;
		if (~full == 0) run = (t >> 1) + 4 * 63;
		else {
			const int f = __builtin_ctzll(~full), cf = __builtin_amdgcn_readlane(cnt, f);
			run = f == 0 ? cf : (t >> 1) + 4 * (f - 1) + cf;
		}
		const int lim = i < j ? i : j;
		run = run < lim ? run : lim;
		const int L = 1 + run;
		for (int q2 = lane; q2 < L; q2 += 64) rev[k + q2] = (uint8_t)'M';
		k += L; i -= L; j -= L;
	}
	for (int q2 = lane; q2 <= i; q2 += 64) rev[k + q2] = (uint8_t)'D';
	k += i >= 0 ? i + 1 : 0;
	for (int q2 = lane; q2 <= j; q2 += 64) rev[k + q2] = (uint8_t)'I';
	k += j >= 0 ? j + 1 : 0;
	if (lane == 0) *len_out = k;
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
	for (int q2 = lane; q2 < k; q2 += 64) op[q2] = rev[k - 1 - q2];
}

template <bool HASN>
__device__ __forceinline__ void band_forward(BandState &S, const u32 *__restrict__ Q, const u32 *__restrict__ R, u32 *dirx, u32 *diry, bool hy, int S8, int G8,
                                             int sfx, int lfx, int sfy, int lfy, int lane)
{
	u32 c1 = 0x00010001u, c2 = 0x00020002u, c4 = 0x00040004u, c16 = 0x00100010u, cm2 = 0xfffefffeu;
	BAND_OPAQUE(c1); BAND_OPAQUE(c2); BAND_OPAQUE(c4); BAND_OPAQUE(c16); BAND_OPAQUE(cm2);
	const u32 *qp = Q + lane, *rp = R + 64 - lane;
	BandQuad cq = *(const BandQuad *)qp, cr = *(const BandQuad *)rp;
	for (int s0 = 0; s0 < S8; s0 += 8) {
		// (the next chunk's codes: the strings reach one chunk past the last step)
		const BandQuad nq = *(const BandQuad *)(qp + (s0 >> 1) + 4), nr = *(const BandQuad *)(rp + (s0 >> 1) + 4);
		const u32 q[5] = { cq.a, cq.b, cq.c, cq.d, nq.a }, r[4] = { cr.a, cr.b, cr.c, cr.d };
		const bool cap = (sfx >= s0 && sfx < s0 + 8) || (sfy >= s0 && sfy < s0 + 8);
		if (s0 < G8) band_chunk<HASN, true, true>(S, s0, q, r, c1, c2, c4, c16, cm2, sfx, lfx, sfy, lfy);
		else if (cap) band_chunk<HASN, false, true>(S, s0, q, r, c1, c2, c4, c16, cm2, sfx, lfx, sfy, lfy);
		else band_chunk<HASN, false, false>(S, s0, q, r, c1, c2, c4, c16, cm2, sfx, lfx, sfy, lfy);
		const size_t at = ((size_t)(s0 >> 3) << 6) + lane;
		dirx[at] = __builtin_amdgcn_perm(S.acc, S.r0, 0x05040100u);
		if (hy) diry[at] = __builtin_amdgcn_perm(S.acc, S.r0, 0x07060302u);
		cq = nq; cr = nr;
	}
}

__global__ void __launch_bounds__(256) k_dp_band(const BandJob *__restrict__ jobs, i32 npairs, const u32 *__restrict__ seq, const u32 *__restrict__ hasn, uint8_t *dirbase,
                                                 uint8_t *revbase, uint8_t *ops, const i64 *__restrict__ ops_off, i32 *ops_len, u32 *cert, u32 tag, i32 B, unsigned long long *ncert)
{
	const int lane = threadIdx.x & 63, p = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (p >= npairs) return;
	const BandJob X = jobs[2 * p], Y0 = jobs[2 * p + 1];
	const bool hy = Y0.job >= 0;
	BandJob Y = Y0;
	if (!hy) { Y = X; Y.job = -1; }      // (a last job without a partner: the high halves compute it once more and keep nothing)
	const int S8 = band_steps8(X, Y0), LQ = band_seq_len(S8);
	const u32 *Q = seq + X.seqoff, *R = Q + LQ;
	// the step that computes a job's last cell, and the lane that holds it
	const int sfx = X.m + X.n, lfx = (X.n - X.m - X.base) >> 1, sfy = Y.m + Y.n, lfy = (Y.n - Y.m - Y.base) >> 1;
	// GUARD chunks: until every lane's cells have i >= 0 (lane 0: s >= 2 - base) and j >= 0 (lane 63: s >= 128 + base)
	int g = 2 - X.base > 128 + X.base ? 2 - X.base : 128 + X.base;
	g = 2 - Y.base > g ? 2 - Y.base : g; g = 128 + Y.base > g ? 128 + Y.base : g;
	const int G8 = (g + 1 + 7) & ~7;
	BandState S;
	S.h1e = S.h1o = S.ee = S.fe = S.eo = S.fo = BAND_NEG2; S.acc = S.r0 = 0; S.capx = S.capy = BAND_NEG2;
	// the cell of step 0: i = base/2 - 1 + l, j = -1 - base/2 - l
	S.iv = (u32)((X.base / 2 - 1 + lane) & 0xffff) | ((u32)((Y.base / 2 - 1 + lane) & 0xffff) << 16);
	S.jv = (u32)((-1 - X.base / 2 - lane) & 0xffff) | ((u32)((-1 - Y.base / 2 - lane) & 0xffff) << 16);
	u32 *dirx = (u32 *)(dirbase + X.diroff), *diry = (u32 *)(dirbase + Y.diroff);
	if (hasn[p]) band_forward<true>(S, Q, R, dirx, diry, hy, S8, G8, sfx, lfx, sfy, lfy, lane);
	else band_forward<false>(S, Q, R, dirx, diry, hy, S8, G8, sfx, lfx, sfy, lfy, lane);
	const int scx = (int)(short)(S.capx & 0xffffu) - 1, scy = (int)(short)(S.capy >> 16) - 1;
	const bool okx = scx > dp_band_ub(X.m, X.n, B), oky = hy && scy > dp_band_ub(Y.m, Y.n, B);
	if (!okx && !oky) return;
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
	if (okx) band_walk(dirx, X.m, X.n, X.base, revbase + ops_off[X.job], ops + ops_off[X.job], ops_len + X.job, lane);
	if (oky) band_walk(diry, Y.m, Y.n, Y.base, revbase + ops_off[Y.job], ops + ops_off[Y.job], ops_len + Y.job, lane);
	if (lane == 0) {
		if (okx) cert[2 * p] = tag;
		if (oky) cert[2 * p + 1] = tag;
		atomicAdd(ncert, (unsigned long long)((okx ? 1 : 0) + (oky ? 1 : 0)));
	}
}

// The default rule (option dp_band = 1): the layout admits the job, and its share of a wave's steps -- (m + n) / 2 with a partner in the other halves --
// is at most three quarters of the wave-steps the cheaper striped form spends on it (stripe_steps).  A band step costs about what a striped step
// costs (24 against 29 VALU instructions for two cells), and a certified job walks back here instead of there; the quarter pays for the forward
// pass of a job that falls back and for the striped kernel's empty workgroup.  dp_band = 2 (tests): every job the layout admits.
bool dp_band_eligible(const gsa_ctx *c, int m, int n, i64 stripe_steps)
{
	if (c->opt.dp_band == 0 || c->dp_safe || !dp_band_fits(m, n, c->opt.dp_band_margin)) return false;
	return c->opt.dp_band == 2 || 2 * (i64)(m + n) <= 3 * stripe_steps;
}

size_t dp_band_table_bytes(size_t njobs) { return (njobs + 2) * sizeof(BandJob); }

// large[idx[k]]: the band jobs of a striped batch, largest m + n first (neighbours share a wave); tab: pinned, dp_band_table_bytes(idx.size()).
// Enqueues the two kernels on st; *cert / *tag: job k's result stands where cert[k] == tag once they have run.
int launch_band(gsa_ctx *c, hipStream_t st, const std::vector<LgJob> &large, const std::vector<i32> &idx, BandJob *tab, const uint8_t *pool1, const i64 *off1, const uint8_t *pool2, const i64 *off2,
                uint8_t *ops, const i64 *ops_off, i32 *ops_len, uint8_t *rev, const u32 **cert_out, u32 *tag_out)
{
	const size_t nj = idx.size(), npairs = (nj + 1) / 2;
	const int B = c->opt.dp_band_margin;
	i64 dbytes = 0, swords = 0;
	for (size_t k = 0; k < 2 * npairs; k++) {
		BandJob &b = tab[k];
		if (k < nj) { const LgJob &g = large[(size_t)idx[k]]; b.job = g.job; b.m = g.m; b.n = g.n; b.base = dp_band_base(g.m, g.n, B); }
		else { b = tab[k - 1]; b.job = -1; }
		b.diroff = 0; b.seqoff = 0;
	}
	for (size_t p = 0; p < npairs; p++) {
		BandJob &x = tab[2 * p], &y = tab[2 * p + 1];
		const int S8 = band_steps8(x, y);
		x.seqoff = y.seqoff = swords; swords += 2 * (i64)band_seq_len(S8);
		x.diroff = dbytes; dbytes += (i64)(S8 / 8) * 256;
		y.diroff = dbytes; if (y.job >= 0) dbytes += (i64)(S8 / 8) * 256;
	}
	uint8_t *dir = dev_ensure<uint8_t>(c, c->d_band_dir, (size_t)dbytes + 256);
	u32 *seq = dev_ensure<u32>(c, c->d_band_seq, (size_t)swords + 64);
	const size_t cert_cap0 = c->d_band_cert.cap;
	u32 *cert = dev_ensure<u32>(c, c->d_band_cert, 3 * npairs + 64);      // a tag per job, then "has an N" per pair
	const bool stat_new = c->d_band_stat.p == nullptr;
	unsigned long long *ncert = dev_ensure<unsigned long long>(c, c->d_band_stat, 2);
	if (!dir || !seq || !cert || !ncert) return GSA_ERR_NOMEM;
	if (stat_new) GSA_CHECK(c, hipMemsetAsync(ncert, 0, 16, st));
	// (a tag is the launch's number: stale flags of earlier launches never match; fresh memory is cleared)
	if (++c->band_epoch == 0 || c->d_band_cert.cap != cert_cap0) { GSA_CHECK(c, hipMemsetAsync(cert, 0, c->d_band_cert.cap, st)); if (c->band_epoch == 0) c->band_epoch = 1; }
	hipLaunchKernelGGL(k_dp_band_prep, dim3((unsigned)npairs), dim3(256), 0, st, (const BandJob *)tab, pool1, off1, pool2, off2, seq, cert + 2 * npairs);
	hipLaunchKernelGGL(k_dp_band, dim3((unsigned)((npairs + 3) / 4)), dim3(256), 0, st, (const BandJob *)tab, (i32)npairs, (const u32 *)seq, (const u32 *)(cert + 2 * npairs), dir,
	                   rev, ops, ops_off, ops_len, cert, c->band_epoch, (i32)B, ncert);
	GSA_CHECK(c, hipGetLastError());
	c->band_eligible += nj;
	*cert_out = cert; *tag_out = c->band_epoch;
	return GSA_OK;
}

// [0] jobs given to the band kernel, [1] of them certified (their results stand), [2] fallen back to the striped kernel
extern "C" int gsa_get_dp_band_stats(gsa_ctx *c, uint64_t st[3])
{
	if (!c || !st) return GSA_ERR_ARG;
	unsigned long long nc = 0;
	if (c->d_band_stat.p) {
		GSA_CHECK(c, hipSetDevice(c->device));
		ctx_quiesce(c);
		GSA_CHECK(c, hipMemcpy(&nc, c->d_band_stat.p, 8, hipMemcpyDeviceToHost));
	}
	st[0] = c->band_eligible; st[1] = nc; st[2] = c->band_eligible - nc;
	return GSA_OK;
}
