// gsalign_amd/csrc/gsa_index.h -- what the two instances of the device index builder share (k_index.hip: up to 2^31 - 2 suffixes, one list, 32-bit suffix numbers;
// k_index_wide.hip: more, in batches, 64-bit suffix numbers): the packed text and its readers, the first-pass key, the builder's device arrays.
#ifndef GSA_INDEX_H
#define GSA_INDEX_H
#include "gsa_scan.h"

#define IX_H0 29
#define IX_T 256

static inline unsigned ix_grid(i64 n) { const i64 g = (n + IX_T - 1) / IX_T; return (unsigned)(g < 1 ? 1 : (g > 16384 ? 16384 : g)); }      // (grid-stride kernels: at most 2^22 work-items per launch)

__device__ __forceinline__ u32 ix_pacsym(const uint8_t *__restrict__ pac, i64 q) { return (u32)(pac[q >> 2] >> ((~q & 3) << 1)) & 3u; }
// the 32 bases from p on, first base in the top bits; the words behind the text are zero
__device__ __forceinline__ u64 ix_get32(const u64 *__restrict__ tw, i64 p)
{
	const i64 wi = p >> 5; const int sh = (int)(p & 31) * 2;
	const u64 a = tw[wi], b = tw[wi + 1];
	return sh ? (a << sh) | (b >> (64 - sh)) : a;
}
__device__ __forceinline__ u32 ix_sym(const u64 *__restrict__ tw, i64 p) { return (u32)(tw[p >> 5] >> (62 - 2 * (int)(p & 31))) & 3u; }
// the 63-bit first-pass key of suffix i: {its first IX_H0 bases, padded with A | min(bases left, IX_H0)} (k_index.hip, END OF TEXT)
__device__ __forceinline__ u64 ix_key0(const u64 *__restrict__ tw, i64 i, i64 S) { const i64 l = S - i; return ((ix_get32(tw, i) >> 6) << 5) | (u64)(l < IX_H0 ? l : IX_H0); }

// T, 2 bits per base, 32 bases per word: the forward strand from .pac, behind it its reverse complement (the text gsah_build_index forms), zeros behind that
static __global__ void __launch_bounds__(IX_T) k_ix_pack(const uint8_t *__restrict__ pac, i64 G, i64 S, u64 *__restrict__ tw, i64 n_tw)
{
	for (i64 w = (i64)blockIdx.x * IX_T + threadIdx.x; w < n_tw; w += (i64)gridDim.x * IX_T) {
		u64 v = 0; const i64 p0 = w * 32;
#pragma unroll 8
		for (int k = 0; k < 32; k++) {
			const i64 p = p0 + k;
			u32 s = 0;
			if (p < G) s = ix_pacsym(pac, p); else if (p < S) s = 3u - ix_pacsym(pac, S - 1 - p);
			v |= (u64)s << (62 - 2 * k);
		}
		tw[w] = v;
	}
}

namespace {
// the builder's device arrays: all freed when the call returns, whichever way (gsa_create_from_pac takes SA out first: release)
struct IxBufs {
	hipStream_t st; std::vector<void *> p;
	~IxBufs() { free_all(); }
	void free_all() { if (p.empty()) return; (void)hipStreamSynchronize(st); for (void *q : p) (void)hipFree(q); p.clear(); (void)hipGetLastError(); }
	void release(void *q) { for (size_t k = 0; k < p.size(); k++) if (p[k] == q) { p.erase(p.begin() + (long)k); return; } }
	template <class T> bool get(T **out, size_t n) { void *q = nullptr; if (hipMalloc(&q, (n ? n : 1) * sizeof(T) + 256) != hipSuccess) { (void)hipGetLastError(); return false; } p.push_back(q); *out = (T *)q; return true; }
};
}

#endif
