// gsalign_amd/csrc/k_index.hip -- the BWT/SA half of the index builder on the device (gsa_build_index): what bwa_idx_build does with BWT-SW
// (BWT_Index/bwtindex.c:77-149, bwt.c:101-123) and host/index_io.cpp with SA-IS / a bucket sorter.  The files of the index are fixed by the suffix ORDER
// of T = forward + reverse complement + '$', so any sorter gives the same bytes; this one is prefix doubling on top of the pipeline's radix sort (gsa_sort.hip):
//   first pass   every suffix gets a 63-bit key {its first IX_H0 = 29 bases, 2 bits each, padded with A = 0 | min(bases left, 29)} and all S keys are sorted.
//                END OF TEXT: '$' sorts before A, so a suffix that runs off the end is smaller than a longer one with the same padded prefix.  The five
//                length bits say exactly that -- shorter first -- and no two suffixes shorter than 29 bases share a key, so each of them is a group of its
//                own from here on (a group's members therefore all have h real bases, and at most one of them ends exactly at '$': rank[S] = 0 below).
//                The order never depends on the order the keys went into the sort in.
//   ranks        rank[i] = the first SA slot of the group of suffixes that tie with i so far; SA[0] = S ('$' alone), rank[S] = 0
//   doubling     h = 29, 58, ...: the suffixes whose group still has more than one member (a list that only shrinks) are sorted by
//                {rank[i], rank[i + h]}, their groups split where that key changes, the new ranks written; the host reads ONE counter per round -- the
//                length of the next list -- and stops at 0.  Rounds ~ log2(longest repeat / 29): no depth limit, no fallback.
// That is the narrow sorter (ix_sort_narrow: 32-bit suffix numbers, one list); the wide one (ix_sort_wide, k_index_wide.hip) does the same in batches with 64-bit
// suffix numbers.  Both start from ix_begin's state and leave an IxBuilt (gsa_index.h), and everything from there on is here ONCE, templated on the SA's element:
// plain passes give what derive_bwt_sa and the interleave loop of host/index_io.cpp give: primary, the 2-bit BWT without the '$' row, its running counts every
// 128 symbols (bwt_bwtupdate_core's layout; scanned in segments with a 64-bit carry, the narrow instance's one segment being the whole text) and the SA samples
// of every 32nd row.  L2 follows from the closing counts.
// gsa_create_from_pac (build_tables_from_pac, at the end) runs the same sort and the same passes for a context: nothing is copied home, the SA array itself becomes the
// context's dense SA (k_ix_widen for the 64-bit layout from the narrow sorter) and the file layout of the BWT words lives only until build_occ (k_tables.hip) has regrouped it.
#include <chrono>
#include "gsa_index.h"

// first-pass keys, two suffixes per thread (S is even): 16-byte key stores, 8-byte value stores
__global__ void __launch_bounds__(IX_T) k_ix_keys0(const u64 *__restrict__ tw, i64 S, u64 *__restrict__ key, u32 *__restrict__ val)
{
	const i64 np = S >> 1;
	for (i64 t = (i64)blockIdx.x * IX_T + threadIdx.x; t < np; t += (i64)gridDim.x * IX_T) {
		const i64 i = 2 * t;
		const i64 l0 = S - i, l1 = l0 - 1;
		ulonglong2 k; uint2 v;
		k.x = ((ix_get32(tw, i) >> 6) << 5) | (u64)(l0 < IX_H0 ? l0 : IX_H0);
		k.y = ((ix_get32(tw, i + 1) >> 6) << 5) | (u64)(l1 < IX_H0 ? l1 : IX_H0);
		v.x = (u32)i; v.y = (u32)(i + 1);
		((ulonglong2 *)key)[t] = k; ((uint2 *)val)[t] = v;
	}
}

// One fused pass over the sorted list of a round (m entries: key, suffix, SA slot; slot = nullptr: entry t sits in slot t + 1, the first pass):
//   component 0  group heads (the key differs from the one in front) -> the group number of every entry, and the slot of every group's head
//   component 1  entries whose group has more than one member -> the next round's list {slot, suffix}, in slot order; its length (cnt: the low half of status word 0)
struct OpIxRound {
	const u64 *key; const u32 *suf; const u32 *slot; i64 m;
	u32 *grp, *head_slot, *slot_out, *suf_out, *cnt;
	struct Item { u32 head, act, slot, suf; };
	__device__ Item load(i64 t) const
	{
		const u64 k = key[t];
		const bool h = t == 0 || key[t - 1] != k, hn = t + 1 >= m || key[t + 1] != k;
		Item it; it.head = h ? 1u : 0u; it.act = (h && hn) ? 0u : 1u; it.slot = slot ? slot[t] : (u32)(t + 1); it.suf = suf[t];
		return it;
	}
	__device__ i32 value(const Item &it, i64, int c) const { return (i32)(c ? it.act : it.head); }
	__device__ void emit(const Item &it, i64 t, const i32 *v, const i32 *ex) const
	{
		const u32 gi = (u32)(ex[0] + v[0] - 1);
		grp[t] = gi;
		if (it.head) head_slot[gi] = it.slot;
		if (it.act) { slot_out[ex[1]] = it.slot; suf_out[ex[1]] = it.suf; }
	}
	__device__ void done(const i32 *tt) const { *cnt = (u32)tt[1]; }
};

// the round's ranks and SA entries: a suffix's rank is the slot of its group's head; the row that holds suffix 0 is primary (the last round that moves it wins)
__global__ void __launch_bounds__(IX_T) k_ix_apply(i64 m, const u32 *__restrict__ suf, const u32 *__restrict__ slot, const u32 *__restrict__ grp, const u32 *__restrict__ head_slot,
                                                   u32 *__restrict__ rank, u32 *__restrict__ SA, u64 *__restrict__ st)
{
	for (i64 t = (i64)blockIdx.x * IX_T + threadIdx.x; t < m; t += (i64)gridDim.x * IX_T) {
		const u32 s = suf[t], sl = slot ? slot[t] : (u32)(t + 1);
		rank[s] = head_slot[grp[t]];
		SA[sl] = s;
		if (s == 0) st[1] = sl;
	}
}

// keys of a doubling round: {rank[i], rank[i + h]}, b bits each; a suffix that ends within h bases has been alone since the first pass, one that ends
// exactly there reads rank[S] = 0, below every other rank
__global__ void __launch_bounds__(IX_T) k_ix_keys(i64 m, const u32 *__restrict__ suf, const u32 *__restrict__ rank, i64 h, i64 S, int b, u64 *__restrict__ key)
{
	for (i64 t = (i64)blockIdx.x * IX_T + threadIdx.x; t < m; t += (i64)gridDim.x * IX_T) {
		const i64 i = suf[t], j = i + h;
		const u32 r1 = rank[i], r2 = rank[j <= S ? j : S];
		key[t] = ((u64)r1 << b) | (u64)(j <= S ? r2 : 0u);
	}
}

// ---- the derivation: from the finished SA (T = u32 or u64 entries) ------------------------------------------------------------------------------------------
// BWT symbol k comes from row i = k + (k >= primary) (derive_bwt_sa, host/index_io.cpp): T[SA[i] - 1], 16 symbols per word, first symbol in the top bits;
// word kw of the plain BWT is word 16 (kw / 8) + 8 + kw % 8 of the interleaved layout.  One symbol per lane, sixteen lanes OR their bits together.
template <class T> __global__ void __launch_bounds__(IX_T) k_ix_bwt(i64 S, const T *__restrict__ SA, const u64 *__restrict__ tw, const u64 *__restrict__ st, u32 *__restrict__ out)
{
	const i64 primary = (i64)st[1];
	for (i64 base = (i64)blockIdx.x * IX_T; base < S; base += (i64)gridDim.x * IX_T) {      // (base is the same in all lanes of a wave: the shuffles below see full waves)
		const i64 k = base + threadIdx.x;
		u32 v = 0;
		if (k < S) {
			const i64 i = k + (k >= primary ? 1 : 0);
			const i64 p = (i64)SA[i] - 1;
			v = ix_sym(tw, p < 0 ? 0 : p) << ((~(u32)k & 15u) << 1);
		}
		v |= __shfl_xor(v, 1); v |= __shfl_xor(v, 2); v |= __shfl_xor(v, 4); v |= __shfl_xor(v, 8);
		if (k < S && (k & 15) == 0) out[(k >> 7) * 16 + 8 + ((k >> 4) & 7)] = v;
	}
}

// running counts in front of every 128-symbol block (four u64: A, C, G, T), two symbols per pass (sym0, sym0 + 1), over the blocks g0 .. g0 + n - 1 of one segment:
// the scan's i32 sums count the segment's symbols only, the counts in front of the segment come in as 64-bit words (carry_in[sym]) and the segment's closing counts
// go out the same way (carry_out: another array, other tiles still read carry_in)
struct OpIxOcc {
	u32 *out; i64 S, n_words, g0; int sym0; const u64 *carry_in; u64 *carry_out;
	struct Item { i32 c0, c1; };
	__device__ Item load(i64 gl) const
	{
		const i64 g = g0 + gl;
		const uint4 *w4 = (const uint4 *)(out + g * 16 + 8);
		const uint4 a = w4[0], b = w4[1];
		const u32 w[8] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w };
		const i64 nw = n_words - g * 8, left = S - g * 128;
		i32 cC = 0, cG = 0, cT = 0;
#pragma unroll
		for (int k = 0; k < 8; k++) {
			const u32 x = k < nw ? w[k] : 0u;      // (behind the last word of the last block lie the closing counts)
			const u32 lo = x & 0x55555555u, hi = (x >> 1) & 0x55555555u;
			cT += __popc(lo & hi); cG += __popc(hi & ~lo); cC += __popc(lo & ~hi);
		}
		const i32 cA = (i32)(left < 128 ? left : 128) - cC - cG - cT;      // (the padding of the last word is zeros, not A's)
		Item it;
		if (sym0 == 0) { it.c0 = cA; it.c1 = cC; } else { it.c0 = cG; it.c1 = cT; }
		return it;
	}
	__device__ i32 value(const Item &it, i64, int c) const { return c ? it.c1 : it.c0; }
	__device__ void emit(const Item &, i64 gl, const i32 *, const i32 *ex) const
	{
		const u64 x0 = carry_in[sym0] + (u64)(u32)ex[0], x1 = carry_in[sym0 + 1] + (u64)(u32)ex[1];
		uint4 o; o.x = (u32)x0; o.y = (u32)(x0 >> 32); o.z = (u32)x1; o.w = (u32)(x1 >> 32);
		*(uint4 *)(out + (g0 + gl) * 16 + 2 * sym0) = o;
	}
	__device__ void done(const i32 *tt) const { carry_out[sym0] = carry_in[sym0] + (u64)(u32)tt[0]; carry_out[sym0 + 1] = carry_in[sym0 + 1] + (u64)(u32)tt[1]; }
};
// the closing counts behind the last block
__global__ void k_ix_close(const u64 *carry, u32 *out, i64 k_end)
{
	const int k = threadIdx.x;
	if (blockIdx.x == 0 && k < 4) { out[k_end + 2 * k] = (u32)carry[k]; out[k_end + 2 * k + 1] = (u32)(carry[k] >> 32); }
}

// sa[j] = SA[32 j], sa[0] = -1 (bwt_cal_sa, bwt.c:101-123)
template <class T> __global__ void __launch_bounds__(IX_T) k_ix_samples(i64 n_sa, const T *__restrict__ SA, u64 *__restrict__ sa)
{
	for (i64 j = (i64)blockIdx.x * IX_T + threadIdx.x; j < n_sa; j += (i64)gridDim.x * IX_T) sa[j] = j ? (u64)SA[32 * j] : ~0ull;
}

// the dense SA of the >= 2^32-row layout (GSA_CREATE_WIDE) from the narrow sorter's array (the only instantiation: a 64-bit SA is adopted as it is); row 0 is the
// sa[0] = -1 sentinel there, SA[0] = S here
template <class T> __global__ void __launch_bounds__(IX_T) k_ix_widen(i64 n, const T *__restrict__ SA, u64 *__restrict__ d64)
{
	for (i64 i = (i64)blockIdx.x * IX_T + threadIdx.x; i < n; i += (i64)gridDim.x * IX_T) d64[i] = i ? (u64)SA[i] : ~0ull;
}

// What the two sorters do alike up front: the geometry, the arrays the derivation reads, the upload, the zeroing, the packed text.  pac: host, ceil(G / 4) bytes.
// rank and everything else only the rounds need are the sorter's own (the hipMalloc calls this puts behind ev0 do not show in the device time: DESIGN.md 8d.1).
int ix_begin(gsa_ctx *c, IxBuilt &X, const uint8_t *pac, i64 G, bool sa64, bool samples, hipEvent_t ev0, const char *who)
{
	const i64 S = 2 * G, n = S + 1;
	X.G = G; X.S = S; X.n = n; X.sa64 = sa64;
	X.n_tw = S / 32 + 3; X.n_words = (S + 15) / 16; X.n_blk = (S + 127) / 128; X.n_bwt = X.n_words + (X.n_blk + 1) * 8; X.n_sa = (S + 32) / 32; X.k_end = X.n_blk * 8 + X.n_words;
	const size_t pac_bytes = (size_t)((G + 3) / 4), bwt_alloc = (size_t)((X.n_bwt + 15) / 16) * 16 + 16;
	hipStream_t st = c->stream;
	IxBufs &B = X.B; B.st = st;
	{ size_t fr = 0, tot = 0; if (hipMemGetInfo(&fr, &tot) != hipSuccess) { (void)hipGetLastError(); fr = 0; } X.free0 = X.free_min = fr; }
	uint8_t *SA;
	if (!B.get(&X.d_pac, pac_bytes) || !B.get(&X.tw, (size_t)X.n_tw) || !B.get(&SA, ((size_t)n + 32) * (sa64 ? 8 : 4)) || !B.get(&X.d_st, (size_t)2) || !B.get(&X.carry, (size_t)8) ||
	    !B.get(&X.d_bwt, bwt_alloc) || (samples && !B.get(&X.d_sa, (size_t)X.n_sa)))
		return gsa_fail(c, GSA_ERR_NOMEM, X.nomem(who) + ")");
	X.SA = SA;
	GSA_CHECK(c, hipMemcpyAsync(X.d_pac, pac, pac_bytes, hipMemcpyHostToDevice, st));
	if (ev0) GSA_CHECK(c, hipEventRecord(ev0, st));
	GSA_CHECK(c, hipMemsetAsync(X.d_bwt, 0, bwt_alloc * 4, st));
	GSA_CHECK(c, hipMemsetAsync(X.carry, 0, 64, st));
	hipLaunchKernelGGL(k_ix_pack, dim3(ix_grid(X.n_tw)), dim3(IX_T), 0, st, (const uint8_t *)X.d_pac, G, S, X.tw, X.n_tw);
	GSA_CHECK(c, hipGetLastError());
	return GSA_OK;
}

// Device bytes per suffix (S = 2G of them): keys 2 x 8, suffixes 2 x 4, slots 2 x 4, rank 4, SA 4, the sort's scratch 12 (c->tmp) + its histograms -- 52 bytes, and
// under 1 byte for the packed text, the BWT words and the samples.
int ix_sort_narrow(gsa_ctx *c, IxBuilt &X, const char *who)
{
	const i64 S = X.S, n = X.n;
	const int b = ceil_log2_u64((u64)S + 1);      // bits of a rank (0 .. S)
	hipStream_t st = c->stream;
	IxBufs &B = X.B;
	u64 *keyA, *keyB; u32 *valA, *valB, *slotA, *slotB, *rank, *SA = (u32 *)X.SA, *d_cnt = (u32 *)X.d_st;
	if (!B.get(&keyA, (size_t)n) || !B.get(&keyB, (size_t)n) || !B.get(&valA, (size_t)n) || !B.get(&valB, (size_t)n) || !B.get(&slotA, (size_t)n) || !B.get(&slotB, (size_t)n) || !B.get(&rank, (size_t)n + 1))
		return gsa_fail(c, GSA_ERR_NOMEM, X.nomem(who) + ")");
	X.dead = { (void *)keyA, (void *)keyB, (void *)valA, (void *)valB, (void *)slotA, (void *)slotB, (void *)rank };
	hipLaunchKernelGGL(k_ix_init<u32>, dim3(1), dim3(64), 0, st, rank, SA, X.d_st, S);
	GSA_CHECK(c, hipGetLastError());
	hipLaunchKernelGGL(k_ix_keys0, dim3(ix_grid(S / 2)), dim3(IX_T), 0, st, (const u64 *)X.tw, S, keyA, valA);
	GSA_CHECK(c, hipGetLastError());
	if (int rc = gsa_sort_pairs_u64_u32(c, keyA, keyB, valA, valB, (size_t)S, 0, 2 * IX_H0 + 5)) return rc;
	// the group numbers and the head slots of a round live where the sort's input keys were (dead once sorted): m + m words
	u32 *grp = (u32 *)keyA, *head_slot = grp + n;
	const u32 *slot = nullptr; u32 *slot_out = slotA;
	i64 m = S, h = IX_H0; i32 nr = 0;
	for (;;) {
		OpIxRound op = { keyB, valB, slot, m, grp, head_slot, slot_out, valA, d_cnt };
		if (int rc = lb_launch<2>(c, m, op, st)) return rc;
		hipLaunchKernelGGL(k_ix_apply, dim3(ix_grid(m)), dim3(IX_T), 0, st, m, (const u32 *)valB, slot, (const u32 *)grp, (const u32 *)head_slot, rank, SA, X.d_st);
		GSA_CHECK(c, hipGetLastError());
		u32 left = 0;
		GSA_CHECK(c, hipMemcpyAsync(&left, d_cnt, 4, hipMemcpyDeviceToHost, st));
		GSA_CHECK(c, hipStreamSynchronize(st));
		if (left == 0) break;
		if (++nr > 64) return gsa_fail(c, GSA_ERR_STATE, std::string("internal: ") + who + ": the suffix groups do not resolve");
		m = (i64)left;
		hipLaunchKernelGGL(k_ix_keys, dim3(ix_grid(m)), dim3(IX_T), 0, st, m, (const u32 *)valA, (const u32 *)rank, h, S, b, keyA);
		GSA_CHECK(c, hipGetLastError());
		if (int rc = gsa_sort_pairs_u64_u32(c, keyA, keyB, valA, valB, (size_t)m, 0, 2 * b)) return rc;
		slot = slot_out; slot_out = slot_out == slotA ? slotB : slotA;
		h *= 2;
	}
	X.rounds = nr;
	return GSA_OK;
}

// the sorter the options name, from the .pac bytes on the host to the finished SA
static int ix_sort(gsa_ctx *c, IxBuilt &X, const uint8_t *pac, i64 G, const IxOpts &o, bool samples, hipEvent_t ev0, const char *who)
{
	if (int rc = ix_begin(c, X, pac, G, o.wide, samples, ev0, who)) return rc;
	return o.wide ? ix_sort_wide(c, X, o.batch_cap, o.active_cap, who) : ix_sort_narrow(c, X, who);
}
// (the narrow instance's one segment: S <= 2^31 - 3, so the whole text's totals fit the scan's i32)
static i64 ix_occ_segment(const IxBuilt &X, const IxOpts &o) { return o.wide ? ixw_seg(o.occ_segment) : X.n_blk; }

static void ix_drop_scratch(gsa_ctx *c) { if (c->tmp.p) { ctx_quiesce(c); (void)hipFree(c->tmp.p); c->tmp.p = nullptr; c->tmp.cap = 0; c->tmp.len = 0; } }

// Everything the rounds used is dead once the sorter returns -- keys, values, slots, ranks, batch arrays, active lists, the sort scratch that grew inside the context: the
// derivation reads SA, the packed text and the .pac bytes only.  gsa_create_from_pac frees them here, BEFORE the context's Occ blocks and samples are allocated (a list
// that was cut to the free memory leaves no room for them otherwise); the index-file builds let them go with the rest when they return, outside their timed region.
static int ix_release_sort(gsa_ctx *c, IxBuilt &X)
{
	GSA_CHECK(c, hipStreamSynchronize(c->stream));
	for (void *q : X.dead) { X.B.release(q); (void)hipFree(q); }
	(void)hipGetLastError();
	X.dead.clear();
	ix_drop_scratch(c);
	return GSA_OK;
}

// the file layout of the .bwt words into X.d_bwt: the symbols, then the running counts in front of every block, segment by segment, and the closing counts
static int ix_bwt_occ(gsa_ctx *c, IxBuilt &X, i64 occ_segment)
{
	hipStream_t st = c->stream;
	if (X.sa64) hipLaunchKernelGGL(k_ix_bwt<u64>, dim3(ix_grid(X.S)), dim3(IX_T), 0, st, X.S, (const u64 *)X.SA, (const u64 *)X.tw, (const u64 *)X.d_st, X.d_bwt);
	else hipLaunchKernelGGL(k_ix_bwt<u32>, dim3(ix_grid(X.S)), dim3(IX_T), 0, st, X.S, (const u32 *)X.SA, (const u64 *)X.tw, (const u64 *)X.d_st, X.d_bwt);
	GSA_CHECK(c, hipGetLastError());
	int par = 0;
	for (i64 g0 = 0; g0 < X.n_blk; g0 += occ_segment, par ^= 1) {
		const i64 ng = X.n_blk - g0 < occ_segment ? X.n_blk - g0 : occ_segment;
		for (int sym0 = 0; sym0 < 4; sym0 += 2) { OpIxOcc op = { X.d_bwt, X.S, X.n_words, g0, sym0, X.carry + 4 * par, X.carry + 4 * (par ^ 1) }; if (int rc = lb_launch<2>(c, ng, op, st)) return rc; }
	}
	hipLaunchKernelGGL(k_ix_close, dim3(1), dim3(64), 0, st, (const u64 *)(X.carry + 4 * par), X.d_bwt, X.k_end);
	GSA_CHECK(c, hipGetLastError());
	return GSA_OK;
}

static int ix_samples(gsa_ctx *c, const IxBuilt &X, u64 *sa)
{
	if (X.sa64) hipLaunchKernelGGL(k_ix_samples<u64>, dim3(ix_grid(X.n_sa)), dim3(IX_T), 0, c->stream, X.n_sa, (const u64 *)X.SA, sa);
	else hipLaunchKernelGGL(k_ix_samples<u32>, dim3(ix_grid(X.n_sa)), dim3(IX_T), 0, c->stream, X.n_sa, (const u32 *)X.SA, sa);
	GSA_CHECK(c, hipGetLastError());
	return GSA_OK;
}

// primary, L2[5], bwt[bwt_words], sa[n_sa]: host.  out->batches: those that hold a suffix; out->peak: device bytes in use at the low-water mark of hipMemGetInfo, less
// what was in use at the start (both 0, like out->active, from the narrow sorter)
int build_index_device(gsa_ctx *c, const uint8_t *pac, i64 G, const IxOpts &o, const char *who, u64 *primary, u64 L2[5], u32 *bwt, u64 *sa, IxStats *out)
{
	hipStream_t st = c->stream;
	hipEvent_t ev[2] = { nullptr, nullptr };
	struct EvGuard { hipEvent_t *e; ~EvGuard() { for (int k = 0; k < 2; k++) if (e[k]) (void)hipEventDestroy(e[k]); } } evg{ ev };
	IxBuilt X;      // (behind the events: its arrays are freed, after a wait for the stream, before they are destroyed)
	GSA_CHECK(c, hipEventCreate(&ev[0])); GSA_CHECK(c, hipEventCreate(&ev[1]));
	if (int rc = ix_sort(c, X, pac, G, o, true, ev[0], who)) return rc;
	if (int rc = ix_bwt_occ(c, X, ix_occ_segment(X, o))) return rc;
	if (int rc = ix_samples(c, X, X.d_sa)) return rc;
	const i64 S = X.S, n_bwt = X.n_bwt, n_sa = X.n_sa, k_end = X.k_end;
	GSA_CHECK(c, hipEventRecord(ev[1], st));
	u64 h_st[2] = { 0, 0 }; i32 lberr = 0;
	GSA_CHECK(c, hipMemcpyAsync(h_st, X.d_st, 16, hipMemcpyDeviceToHost, st));
	GSA_CHECK(c, hipMemcpyAsync(&lberr, c->d_mail.as<i32>() + M_LBERR, 4, hipMemcpyDeviceToHost, st));
	GSA_CHECK(c, hipMemcpyAsync(bwt, X.d_bwt, (size_t)n_bwt * 4, hipMemcpyDeviceToHost, st));
	GSA_CHECK(c, hipMemcpyAsync(sa, X.d_sa, (size_t)n_sa * 8, hipMemcpyDeviceToHost, st));
	GSA_CHECK(c, hipStreamSynchronize(st));
	if (lberr) return gsa_fail(c, GSA_ERR_STATE, "internal: look-back scan timed out");
	if (X.sa64) X.mark();
	float fms = 0; if (hipEventElapsedTime(&fms, ev[0], ev[1]) != hipSuccess) { fms = 0; (void)hipGetLastError(); }
	*primary = h_st[1];
	L2[0] = 0;
	for (int k = 0; k < 4; k++) L2[k + 1] = L2[k] + ((u64)bwt[k_end + 2 * k] | ((u64)bwt[k_end + 2 * k + 1] << 32));
	if (L2[4] != (u64)S) return gsa_fail(c, GSA_ERR_STATE, std::string("internal: ") + who + ": the symbol counts do not add up");
	out->ms = (double)fms; out->rounds = X.rounds; out->batches = X.batches; out->active = X.active; out->peak = (u64)(X.free0 - X.free_min);
	return GSA_OK;
}

// gsa_create_from_pac's device half: the index tables of a context straight from the sort, with no copy home and no LF walk.  The caller has set up the
// context's own state, the chromosome tables, d_ref (2G + 64 bytes) and force_wide (implied by the wide sorter); this fills di.primary / L2 / seq_len, the Occ blocks
// (build_occ from the file layout in a short-lived device buffer), the sampled SA, RefSequence (unpack_pac from the .pac bytes the sort uploaded) and the dense SA -- the
// builder's own SA array, adopted as d_sa_dense (row 0 patched to the -1 sentinel) or, 32-bit entries for the 64-bit layout (GSA_CREATE_WIDE), widened into it.
// Everything else the builder allocated is freed before it returns, the sort scratch that grew inside the context included: the caller chooses the k-mer table's size
// from the free device memory next.
int build_tables_from_pac(gsa_ctx *c, const uint8_t *pac, i64 G, const IxOpts &o)
{
	hipStream_t st = c->stream;
	IxBuilt X;
	struct ScratchGuard { gsa_ctx *c; ~ScratchGuard() { ix_drop_scratch(c); } } sg{ c };
	if (int rc = ix_sort(c, X, pac, G, o, false, nullptr, "gsa_create_from_pac")) return rc;
	if (int rc = ix_release_sort(c, X)) return rc;
	if (int rc = ix_bwt_occ(c, X, ix_occ_segment(X, o))) return rc;
	const i64 S = X.S, n = X.n, n_sa = X.n_sa;
	u64 h_st[2] = { 0, 0 }; u32 h_end[8] = { 0, 0, 0, 0, 0, 0, 0, 0 }; i32 lberr = 0;
	GSA_CHECK(c, hipMemcpyAsync(h_st, X.d_st, 16, hipMemcpyDeviceToHost, st));
	GSA_CHECK(c, hipMemcpyAsync(h_end, X.d_bwt + X.k_end, 32, hipMemcpyDeviceToHost, st));
	GSA_CHECK(c, hipMemcpyAsync(&lberr, c->d_mail.as<i32>() + M_LBERR, 4, hipMemcpyDeviceToHost, st));      // (no fused pass runs below this point)
	GSA_CHECK(c, hipStreamSynchronize(st));
	if (lberr) return gsa_fail(c, GSA_ERR_STATE, "internal: look-back scan timed out");
	c->di.primary = h_st[1]; c->di.L2[0] = 0;
	for (int k = 0; k < 4; k++) c->di.L2[k + 1] = c->di.L2[k] + ((u64)h_end[2 * k] | ((u64)h_end[2 * k + 1] << 32));
	if (c->di.L2[4] != (u64)S) return gsa_fail(c, GSA_ERR_STATE, "internal: gsa_create_from_pac: the symbol counts do not add up");
	c->di.seq_len = (u64)S;
	if (int rc = build_occ(c, X.d_bwt, (u64)((X.n_bwt + 15) / 16))) return rc;
	if (hipMalloc(&c->d_sa.p, (size_t)n_sa * 8) != hipSuccess) { (void)hipGetLastError(); return gsa_fail(c, GSA_ERR_NOMEM, "hipMalloc (sampled SA)"); }
	c->d_sa.cap = (size_t)n_sa * 8;
	if (int rc = ix_samples(c, X, c->d_sa.as<u64>())) return rc;
	c->di.sa = c->d_sa.as<u64>();
	if (int rc = unpack_pac(c, X.d_pac, G, c->d_ref.as<uint8_t>())) return rc;
	// all but SA go now (a widened array is allocated into the room they leave)
	X.B.release(X.SA);
	struct SaGuard { void *p; hipStream_t st; ~SaGuard() { if (p) { (void)hipStreamSynchronize(st); (void)hipFree(p); (void)hipGetLastError(); } } } sag{ X.SA, st };
	X.B.free_all();
	ix_drop_scratch(c);
	if (X.sa64 || !c->force_wide) {
		const size_t w = X.sa64 ? 8 : 4;
		GSA_CHECK(c, hipMemsetAsync(X.SA, 0xFF, w, st));      // row 0: SA[0] = S here, the sa[0] = -1 sentinel there
		c->d_sa_dense.p = X.SA; c->d_sa_dense.len = ((size_t)n + 32) * w; c->d_sa_dense.cap = c->d_sa_dense.len + 256; sag.p = nullptr;      // (IxBufs::get's size is dev_ensure's exact size)
		c->di.sa32 = X.sa64 ? nullptr : c->d_sa_dense.as<u32>(); c->di.sa64 = X.sa64 ? c->d_sa_dense.as<u64>() : nullptr;
	} else {
		if (!dev_ensure<u64>(c, c->d_sa_dense, (size_t)n + 32, true)) return GSA_ERR_NOMEM;
		hipLaunchKernelGGL(k_ix_widen<u32>, dim3(ix_grid(n)), dim3(IX_T), 0, st, n, (const u32 *)X.SA, c->d_sa_dense.as<u64>());
		GSA_CHECK(c, hipGetLastError());
		c->di.sa64 = c->d_sa_dense.as<u64>(); c->di.sa32 = nullptr;
	}
	GSA_CHECK(c, hipStreamSynchronize(st));
	return GSA_OK;
}
