// tests/dp_band_host.cpp -- the band DP's shared header (gsalign_amd/csrc/gsa_dp.h, -DGSA_DP_HOST) behind a C interface for tests/test_dp_band_host.py:
// the host twin of k_dp_band, and a check of the certificate's bound that knows nothing of the band code.
#include <algorithm>
#include <cstdint>
#include <random>
#include <utility>
#include <vector>
#include "gsa_dp.h"

static std::vector<uint8_t> codes(const uint8_t *s, int n)
{
	std::vector<uint8_t> c((size_t)n);
	for (int i = 0; i < n; i++) { const char ch = (char)(s[i] | 0x20); c[(size_t)i] = ch == 'a' ? 0 : ch == 'c' ? 1 : ch == 'g' ? 2 : ch == 't' ? 3 : 4; }
	return c;
}

// s1 / s2: bases.  window = 0: the band [lo, hi] of margin B itself; 1: the window the kernel evaluates.  Returns 1 if the band score exceeds UB.
extern "C" int band_align(const uint8_t *s1, int m, const uint8_t *s2, int n, int B, int window, uint8_t *ops, int *nops, int *score)
{
	const std::vector<uint8_t> c1 = codes(s1, m), c2 = codes(s2, n);
	const int lo = window ? dp_band_base(m, n, B) : dp_band_lo(m, n, B), hi = window ? lo + DP_BAND_DIAGS - 1 : dp_band_hi(m, n, B);
	std::vector<uint8_t> o;
	*score = dp_band_align_host(c1.data(), m, c2.data(), n, lo, hi, o);
	*nops = (int)o.size();
	std::copy(o.begin(), o.end(), ops);
	return *score > dp_band_ub(m, n, B) ? 1 : 0;
}
extern "C" int band_fits(int m, int n, int B) { return dp_band_fits(m, n, B) ? 1 : 0; }
extern "C" int band_ub(int m, int n, int B) { return dp_band_ub(m, n, B); }

// The best global score (match 1, mismatch -1, N 0, a gap of k costs 2 + k) of a path that passes through at least one cell -- boundary cells
// included -- whose diagonal i - j lies outside [lo, hi]: the full-matrix recurrence with the state doubled by "has been outside".
static int best_outside(const std::vector<uint8_t> &s1, const std::vector<uint8_t> &s2, int lo, int hi)
{
	const int m = (int)s1.size(), n = (int)s2.size(), NEG = -1000000, W = n + 1;
	auto at = [&](int i, int j) { return (size_t)(j + 1) * W + (i + 1); };
	auto out = [&](int i, int j) { return i - j < lo || i - j > hi; };
	std::vector<int> H[2], E[2], F[2];
	for (int t = 0; t < 2; t++) { H[t].assign((size_t)(m + 1) * W, NEG); E[t] = H[t]; F[t] = H[t]; }
	H[0][at(-1, -1)] = 0;
	bool was = false;
	for (int i = 0; i < n; i++) { was = was || out(i, -1); H[was][at(i, -1)] = -(3 + i); F[was][at(i, 0)] = -(3 + i) - 3; }
	was = false;
	for (int j = 0; j < m; j++) { was = was || out(-1, j); H[was][at(-1, j)] = -(3 + j); E[was][at(0, j)] = -(3 + j) - 3; }
	for (int j = 0; j < m; j++)
		for (int i = 0; i < n; i++) {
			const int sc = dp_band_sub(s2[(size_t)i], s1[(size_t)j]);
			int hd[2], e[2], f[2];
			for (int t = 0; t < 2; t++) { hd[t] = H[t][at(i - 1, j - 1)] + sc; e[t] = E[t][at(i, j)]; f[t] = F[t][at(i, j)]; }
			if (out(i, j)) { hd[1] = std::max(hd[0], hd[1]); e[1] = std::max(e[0], e[1]); f[1] = std::max(f[0], f[1]); hd[0] = e[0] = f[0] = NEG; }
			for (int t = 0; t < 2; t++) {
				const int h = std::max(hd[t], std::max(e[t], f[t]));
				H[t][at(i, j)] = h < NEG ? NEG : h;
				if (i + 1 < n) E[t][at(i + 1, j)] = std::max(NEG, std::max(e[t], h - 2) - 1);
				if (j + 1 < m) F[t][at(i, j + 1)] = std::max(NEG, std::max(f[t], h - 2) - 1);
			}
		}
	return H[1][at(n - 1, m - 1)];
}

// random small pairs (related, unrelated, with N): how many have a path through an out-of-band cell that scores above UB (0 if the bound holds);
// *reached counts the pairs where such a path exists at all, *tight those where it scores exactly UB
extern "C" int band_bound_violations(int trials, unsigned seed, int *reached, int *tight)
{
	std::mt19937 rng(seed);
	int bad = 0; *reached = 0; *tight = 0;
	for (int k = 0; k < trials; k++) {
		const int m = 1 + (int)(rng() % 40), B = 1 + (int)(rng() % 6);
		int n = (rng() & 1) ? 1 + (int)(rng() % 40) : std::max(1, std::min(40, m + (int)(rng() % 9) - 4));
		std::vector<uint8_t> s1((size_t)m), s2((size_t)n);
		const int alpha = (rng() % 4 == 0) ? 1 + (int)(rng() % 2) : 4;      // (one- and two-letter texts: ties and long cheap excursions)
		for (auto &c : s1) c = (uint8_t)(rng() % alpha);
		for (int i = 0; i < n; i++) s2[(size_t)i] = (k % 3 == 0) ? (uint8_t)(rng() % alpha) : s1[(size_t)std::min(i, m - 1)];
		if (k % 3 == 1) for (int q = 0; q < 3; q++) s2[rng() % n] = (uint8_t)(rng() % alpha);
		if (k % 7 == 0) { s1[rng() % m] = 4; s2[rng() % n] = 4; }
		const int best = best_outside(s1, s2, dp_band_lo(m, n, B), dp_band_hi(m, n, B)), ub = dp_band_ub(m, n, B);
		if (best > -1000000 / 2) (*reached)++;
		if (best == ub) (*tight)++;
		if (best > ub) bad++;
	}
	return bad;
}
