// gsalign_amd/csrc/gsa_dp.h -- device-side global affine-gap DP with traceback (a13).
//
// Restates ksw_extz2_sse + ksw_backtrack as called by ksw2_alignment
// (reference src/ksw2_alignment.cpp:25-68,70-249,251-273): m=5, q=2, e=1, w=-1,
// i.e. full matrix, match +1, mismatch -1, N 0, gap k costs 2+k.  Suzuki-Kasahara
// difference recurrence, one byte of direction flags per cell, exact tie rules
// (diagonal beats a, a beats b), cell-exact (no SIMD padding): SURVEY.md App. A.6.
// s1 = reference fragment (ksw "query", index j, length m), s2 = query fragment
// (ksw "target", index i = t, length n); anti-diagonal r = i + j.
// No MFMA: this is 8-bit max/add with a data-dependent traceback.
//
// -DGSA_DP_HOST: the part shared with the band kernel (k_dp_band.hip) -- cell in absolute scores, layout, certificate,
// traceback automaton -- and a host twin of that kernel, for a plain C++ compiler (tests/dp_band_host.cpp).
#ifndef GSA_DP_H
#define GSA_DP_H
#ifdef GSA_DP_HOST
#include <cstdint>
#include <vector>
#define GSA_HD
typedef uint32_t u32;
#else
#include "gsa_fm.h"
#define GSA_HD __host__ __device__

// one cell of the recurrence (ksw2_alignment.cpp:74-95,184-199).
// in : xt1,vt1 = x,v of (r-1,t-1); ut,yt = u,y of (r-1,t); a_,b_ = codes of s2[t], s1[r-t]
// out: new u,v,x,y of (r,t) and the direction byte
__device__ __forceinline__ int dp_cell(int xt1, int vt1, int ut, int yt, int a_, int b_, int &un, int &vn, int &xn, int &yn)
{
	const int sc = (a_ == 4 || b_ == 4) ? 0 : (a_ == b_ ? 1 : -1);
	int z = sc + 6;
	int a = xt1 + vt1, b = yt + ut;
	int d = a > z ? 1 : 0; z = z > a ? z : a;
	if (b > z) d = 2;
	z = z > b ? z : b;
	z = z < 7 ? z : 7;
	un = z - vt1; vn = z - ut;
	z -= 2; a -= z; b -= z;
	if (a > 0) d |= 0x08; else a = 0;
	if (b > 0) d |= 0x10; else b = 0;
	xn = a; yn = b;
	return d;
}

// shift a value one lane up across the whole 64-lane wave (lane t receives lane t-1's value;
// lane 0 receives `fill`): DPP wave_shr:1, a VALU-rate move instead of an LDS round trip
__device__ __forceinline__ int wave_shr1(int v, int fill)
{
	return __builtin_amdgcn_update_dpp(fill, v, 0x138, 0xf, 0xf, false);
}
// ... and one lane down (lane t receives lane t+1's value, lane 63 `fill`): DPP wave_shl:1
__device__ __forceinline__ int wave_shl1(int v, int fill)
{
	return __builtin_amdgcn_update_dpp(fill, v, 0x130, 0xf, 0xf, false);
}
#endif

// the traceback automaton (ksw_backtrack :38-52), branch-free: the state after a cell (0: M, 1: D, 2: I), given
// the state before it and the cell's flag byte; with the full band the force_state paths never fire
GSA_HD inline int dp_bt_next(int state, u32 flags)
{
	if (state != 0 && !((flags >> (state + 2)) & 1)) state = 0;
	if (state == 0) state = (int)(flags & 7);
	return state;
}

// ---------------------------------------------------------------------------
// The diagonal band (k_dp_band.hip).  The same recurrence in ABSOLUTE scores -- H(i,j) = max(H(i-1,j-1) + s, E(i,j), F(i,j)),
// E(i+1,j) = max(E(i,j), H(i,j) - q) - e, F(i,j+1) = max(F(i,j), H(i,j) - q) - e, H(-1,-1) = 0, H(i,-1) = H(-1,i) = -(q + e (i + 1)),
// E(0,j) = H(-1,j) - q - e, F(i,0) = H(i,-1) - q - e -- over the cells whose diagonal i - j lies in a window; everything outside is -infinity.
// With x' = x + q + e (and so on) the difference form above is this one term by term: a' > z' <=> E > H(i-1,j-1) + s, b' > max <=> F > max of the
// two, a' - (z' - q) > 0 <=> E > H - q: the flag byte of a cell is the same function of the same comparisons.
// Scores fit 16 bits: |H| <= 3 * 5000 + 4 for fragments up to DP_BAND_MAX_LEN, and DP_BAND_NEG stands below every one of them.
// ---------------------------------------------------------------------------
#define DP_BAND_DIAGS 128          // diagonals a wave evaluates: lane l owns base + 2l (even steps) and base + 2l + 1 (odd steps)
#define DP_BAND_MAX_LEN 5000       // longest fragment on either side
#define DP_BAND_NEG (-16384)
// flag byte of a cell as dp_cell writes it, from hd = H(i-1,j-1) + s, e = E(i,j), f = F(i,j); out: H(i,j), E(i+1,j), F(i,j+1)
GSA_HD inline int dp_band_cell(int hd, int e, int f, int &h, int &en, int &fn)
{
	int d = 0; h = hd;
	if (e > h) { d = 1; h = e; }
	if (f > h) { d = 2; h = f; }
	const int hq = h - 2;
	if (e > hq) d |= 0x08; else e = hq;
	if (f > hq) d |= 0x10; else f = hq;
	en = e - 1; fn = f - 1;
	return d;
}
GSA_HD inline int dp_band_sub(int a, int b) { return (a >= 4 || b >= 4) ? 0 : (a == b ? 1 : -1); }
// the certified band of an m x n job at margin B: diagonals i - j in [lo, hi]
GSA_HD inline int dp_band_lo(int m, int n, int B) { return (n - m < 0 ? n - m : 0) - B; }
GSA_HD inline int dp_band_hi(int m, int n, int B) { return (n - m > 0 ? n - m : 0) + B; }
// ... and the window the kernel evaluates: DP_BAND_DIAGS diagonals from an even one at or below lo (a wave's two jobs then share the parity of their steps)
GSA_HD inline int dp_band_base(int m, int n, int B) { return dp_band_lo(m, n, B) & ~1; }
GSA_HD inline bool dp_band_fits(int m, int n, int B)
{
	return m >= 1 && n >= 1 && m <= DP_BAND_MAX_LEN && n <= DP_BAND_MAX_LEN && dp_band_hi(m, n, B) - dp_band_base(m, n, B) + 1 <= DP_BAND_DIAGS;
}
// The certificate.  A global path that touches a diagonal above hi climbs there from diagonal 0 and comes back down to n - m: at least
// max(0, n - m) + B + 1 'D' and max(0, n - m) + B + 1 - (n - m) 'I' columns, so two gaps at least (4 for opening them), |n - m| + 2B + 2 gap columns
// (1 each) and at most min(m, n) - (B + 1) diagonal columns (+1 each at best); below lo: the same with the sides exchanged.  Its score is at most
// UB = min(m, n) - |n - m| - 3 (B + 1) - 4: a band score above UB is the optimum, and every optimal path lies inside [lo, hi].
GSA_HD inline int dp_band_ub(int m, int n, int B)
{
	const int d = n - m < 0 ? m - n : n - m;
	return (m < n ? m : n) - d - 3 * (B + 1) - 4;
}

#ifdef GSA_DP_HOST
// Host twin of k_dp_band for one job: the window [dlo, dhi] of diagonals cell by cell, the walk back with dp_bt_next.  s1 / s2: codes 0-4.
// Returns the band score (H of the last cell); ops: the M / D / I string, first column first.
static inline int dp_band_align_host(const uint8_t *s1, int m, const uint8_t *s2, int n, int dlo, int dhi, std::vector<uint8_t> &ops, std::vector<uint8_t> *flags_out = nullptr)
{
	const int NEG = DP_BAND_NEG, W = n + 1;
	std::vector<int> H((size_t)(m + 1) * W, NEG), E((size_t)(m + 1) * W, NEG), F((size_t)(m + 1) * W, NEG);      // index (j + 1) * W + (i + 1): H of (i, j); E, F INTO (i, j)
	std::vector<uint8_t> fl((size_t)m * n, 0xff);
	auto in = [&](int i, int j) { return i - j >= dlo && i - j <= dhi; };
	auto at = [&](int i, int j) { return (size_t)(j + 1) * W + (i + 1); };
	H[at(-1, -1)] = 0;
	for (int i = 0; i < n; i++) if (in(i, -1)) { H[at(i, -1)] = -(3 + i); F[at(i, 0)] = H[at(i, -1)] - 3; }
	for (int j = 0; j < m; j++) if (in(-1, j)) { H[at(-1, j)] = -(3 + j); E[at(0, j)] = H[at(-1, j)] - 3; }
	for (int j = 0; j < m; j++)
		for (int i = 0; i < n; i++) {
			if (!in(i, j)) continue;
			const int hd = H[at(i - 1, j - 1)] + dp_band_sub(s2[i], s1[j]);      // (a neighbour outside the window: NEG, +-1)
			int h, en, fn;
			fl[(size_t)j * n + i] = (uint8_t)dp_band_cell(hd, E[at(i, j)], F[at(i, j)], h, en, fn);
			H[at(i, j)] = h;
			if (i + 1 < n) E[at(i + 1, j)] = en;
			if (j + 1 < m) F[at(i, j + 1)] = fn;
		}
	ops.clear();
	int i = n - 1, j = m - 1, state = 0;
	while (i >= 0 && j >= 0) {
		if (!in(i, j)) { ops.clear(); return NEG; }      // (cannot happen: -infinity never wins)
		state = dp_bt_next(state, fl[(size_t)j * n + i]);
		if (state == 0) { ops.push_back('M'); i--; j--; }
		else if (state == 1 || state == 3) { ops.push_back('D'); i--; }
		else { ops.push_back('I'); j--; }
	}
	for (; i >= 0; --i) ops.push_back('D');
	for (; j >= 0; --j) ops.push_back('I');
	for (size_t a = 0, b = ops.size(); a + 1 < b; a++, b--) std::swap(ops[a], ops[b - 1]);
	if (flags_out) *flags_out = fl;
	return H[at(n - 1, m - 1)];
}
#endif

#endif
