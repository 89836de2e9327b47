// gsalign_amd/csrc/k_dp.hip -- batched gap-closing DP (a13): the jobs of a list sorted into size classes, the classes'
// launches tied together (run_ksw2_jobs), and the public leaf operator gsa_ksw2_batch.  Cell recurrence and traceback
// automaton: gsa_dp.h.
//
// Three classes, one kernel each, chosen per job by size (the small classes run concurrently with the striped kernel):
//  * k_dp_lane    at most `dp_lane` cells (default 512) inside the bounds of k_dp_small: one LANE per alignment.
//  * k_dp_small   n <= 64 and m+n-1 <= 128 (with k_dp_lane the bulk of the jobs: median 11 x 11): one wavefront per
//    alignment.  Both kernels and their launch (launch_small_dp): k_dp_small.hip.
//  * k_dp_stripe  everything else (up to 5000 x 5000): the target columns are cut into 64-wide stripes, one wavefront
//    per PAIR of stripes (packed 16-bit VALU), boundary columns handed over through LDS / HBM.  The kernel and its
//    launch by size class of the reference fragment (launch_stripes): k_dp_stripe.hip.  Its near-diagonal jobs run in
//    k_dp_band first (a window of 128 diagonals, two jobs per wavefront, certified or redone here): k_dp_band.hip.
#include <algorithm>
#include <cstring>
#include "gsa_ctx.h"
#include "gsa_scan.h"
#include "gsa_gap.h"

// Size classes on the device: one fused pass (gsa_scan.h) lists the jobs that need the striped kernel
// as (job, m, n) triples and packs the others into the order arrays of k_dp_lane and k_dp_small.
struct OpClassify {
	const i32 *len1, *len2; i32 *order, *order_lane, *lg, *jlarge, *mail;
	static constexpr bool clamped = true;      // (gsa_scan.h: every element's loads unconditional and together; beyond the job count the lengths are stale, not used)
	struct Item { i32 in, m, n; };
	__device__ Item load(i64 j) const { Item it; it.in = 0; it.m = len1[j]; it.n = len2[j]; return it; }
	__device__ void prep(Item &it, i64 j) const { it.in = j < mail[M_NJOB] ? 1 : 0; if (!it.in) it.m = it.n = 0; }
	__device__ i32 value(const Item &it, i64, int c) const
	{
		if (!it.in) return 0;
		const i32 m = it.m, n = it.n;
		if (c == 0) return dp_is_large(m, n) ? 1 : 0;
		if (dp_is_large(m, n)) return 0;
		return lane_cells > 0 && m * n <= lane_cells ? 1 : 0;           // one lane each (k_dp_lane); the rest of the class: one wavefront each (k_dp_small)
	}
	__device__ void emit(const Item &it, i64 j, const i32 *v, const i32 *ex) const
	{
		if (!it.in) return;
		const i32 m = it.m, n = it.n;
		if (m <= 0 || n <= 0) lb_pub(&mail[M_DPERR], 2);
		jlarge[j] = v[0];
		if (v[0]) { i32 *e = lg + 3 * (size_t)ex[0]; lb_pub(&e[0], (i32)j); lb_pub(&e[1], m); lb_pub(&e[2], n); }      // (finish() reads the list)
		else if (v[1]) order_lane[ex[1]] = (i32)j;
		else order[j - ex[0] - ex[1]] = (i32)j;
	}
	__device__ void done(const i32 *t) const { lb_pub(&mail[M_NLARGE], t[0]); lb_pub(&mail[M_NLANE], t[1]); }
	// the last tile puts the mailbox and the head of the large-job list into pinned memory (the host launches from there)
	i32 *h_out; i32 h_cap; i32 lane_cells;
	__device__ void finish(int tid) const
	{
		if (tid < MAIL_N) h_out[tid] = __hip_atomic_load(&mail[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		i32 nl = __hip_atomic_load(&mail[M_NLARGE], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); if (nl > h_cap) nl = h_cap;
		lb_copy_out(h_out + MAIL_N, lg, 3 * nl, tid);
	}
};

// sums of m*n and m+n over the jobs (measurement only)
__global__ void k_dp_cells(const i32 *__restrict__ mail, const i32 *__restrict__ len1, const i32 *__restrict__ len2, unsigned long long *out)
{
	const i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x;
	const bool in = j < mail[M_NJOB];
	unsigned long long v = in ? (unsigned long long)len1[j] * (unsigned long long)len2[j] : 0, w = in ? (unsigned long long)(len1[j] + len2[j]) : 0;
	for (int o = 32; o; o >>= 1) { v += __shfl_xor(v, o); w += __shfl_xor(w, o); }
	if ((threadIdx.x & 63) == 0 && v) { atomicAdd(out, v); atomicAdd(out + 1, w); }
}

void dp_count_cells(gsa_ctx *c, i32 n_ub, const i32 *len1, const i32 *len2, hipStream_t stream)
{
	hipLaunchKernelGGL(k_dp_cells, dim3(grid_for((size_t)n_ub, 256)), dim3(256), 0, stream, c->d_mail.as<i32>(), len1, len2, (unsigned long long *)(c->d_mail.as<i32>() + M_CELLS));
}

#define LG_CHUNK 2048       // large-job triples copied together with the mailbox (more -> a second copy)

// All pointers are device pointers; the job count sits in mail[M_NJOB] (<= n_ub).  Jobs that do not fit
// the small kernel are processed in batches so that the direction bytes of one batch fit the budget.
// Returns with the work enqueued: errors of the last batch land in the mailbox (M_DPERR, M_DPERR2).
int run_ksw2_jobs(gsa_ctx *c, i32 n_ub, const uint8_t *pool1, const i64 *off1, const i32 *len1,
                  const uint8_t *pool2, const i64 *off2, const i32 *len2, uint8_t *ops, const i64 *ops_off, i32 *ops_len, i64 ops_total, Ksw2Launch *out,
                  const i32 *jfrag, gsa_frag *frag, bool mail_clean)
{
	*out = Ksw2Launch();
	if (n_ub <= 0) return GSA_OK;
	hipStream_t st = c->stream;
	i32 *mail = c->d_mail.as<i32>();
	i32 *d_order = dev_ensure<i32>(c, c->d_flag2, (size_t)n_ub + 2);
	i32 *d_order_lane = dev_ensure<i32>(c, c->d_dp_lane_order, (size_t)n_ub + 2);
	i32 *d_lg = dev_ensure<i32>(c, c->d_dp_large, 4 * ((size_t)n_ub + 1));      // (job, m, n) triples of the large jobs, then one flag per job
	i32 *d_jlarge = d_lg ? d_lg + 3 * ((size_t)n_ub + 1) : nullptr;
	uint8_t *rev = dev_ensure<uint8_t>(c, c->d_i64a, (size_t)ops_total + 64);
	if (!d_order || !d_order_lane || !d_lg || !rev) return GSA_ERR_NOMEM;
	if (!pin_ensure<i32>(c, c->p_dp, (size_t)MAIL_N + 3 * LG_CHUNK)) return GSA_ERR_NOMEM;
	if (!mail_clean) GSA_CHECK(c, hipMemsetAsync(mail + M_DPERR, 0, 8 * sizeof(i32), st));                    // M_DPERR, M_NLARGE, M_DPERR2, -, M_CELLS (2 x u64): one aligned fill (28 bytes at an odd offset were three)
	i32 *h = c->p_dp.as<i32>();
	const size_t first_lg = (size_t)std::min<i64>(n_ub, LG_CHUNK);
	// Size classes below the striped kernel: alignments of at most GSA_DP_LANE cells (default 512; swept 256 .. 8192: profiles/archive/r03_dp_lane_sweep.txt) go one per LANE (k_dp_lane: every lane busy
	// on every instruction; a lane walks its cells one after the other, so the largest job of a launch is its latency floor --
	// 35 instructions per cell), the larger ones one per wavefront (k_dp_small).  GSA_DP_LANE=0: no lane class, all of them one per wavefront.
	{ OpClassify op = { len1, len2, d_order, d_order_lane, d_lg, d_jlarge, mail, h, (i32)first_lg, c->opt.dp_lane }; int rc = lb_launch<2>(c, n_ub, op); if (rc) return rc; }
	GSA_CHECK(c, hipStreamSynchronize(st));
	if (h[M_LBERR]) return gsa_fail(c, GSA_ERR_STATE, "internal: look-back scan timed out");
	if (h[M_DPERR]) return gsa_fail(c, GSA_ERR_ARG, "DP job with an empty side");
	const i32 n = h[M_NJOB], nlarge = h[M_NLARGE], nlane = h[M_NLANE], nsmall = n - nlarge - nlane;
	out->n = n; out->nsmall = nsmall + nlane; out->nlarge = nlarge;
	if (n <= 0) return GSA_OK;
	c->counters[5] += (u64)n;
	if ((size_t)nlarge > first_lg) {
		i32 keep[MAIL_N]; memcpy(keep, h, sizeof(keep));      // the mailbox copy must survive the reallocation (the caller reads it too)
		if (!pin_ensure<i32>(c, c->p_dp, (size_t)MAIL_N + 3 * (size_t)nlarge)) return GSA_ERR_NOMEM;
		h = c->p_dp.as<i32>(); memcpy(h, keep, sizeof(keep));
		GSA_CHECK(c, hipMemcpyAsync(h + MAIL_N, d_lg, (size_t)nlarge * 12, hipMemcpyDeviceToHost, st));
		GSA_CHECK(c, hipStreamSynchronize(st));
	}
	std::vector<LgJob> large((const LgJob *)(h + MAIL_N), (const LgJob *)(h + MAIL_N) + nlarge);
	// the many small jobs run on a second stream, concurrently with the striped ones
	if (nsmall + nlane > 0) {
		int rc = launch_small_dp(c, st, nlane, d_order_lane, nsmall, d_order, pool1, off1, len1, pool2, off2, len2, ops, ops_off, ops_len, jfrag, frag);
		if (rc) return rc;
		out->small_in_flight = true;
	}
	if (nlarge > 0) {
		// (large gaps are normally launched early, from the leaf table; whatever turns up here shares their buffers)
		if (c->early_in_flight) GSA_CHECK(c, hipStreamWaitEvent(st, c->ev[14], 0));
		int rc = launch_stripes(c, st, large, pool1, off1, pool2, off2, ops, ops_off, ops_len, rev, M_DPERR2);
		if (rc) return rc;
	}
	// (no join: the caller decides what else runs behind the small kernel on stream_aux[1]; event ev[12] marks its end)
	return GSA_OK;
}

extern "C" int gsa_ksw2_batch(gsa_ctx *c, int32_t n_pairs, const char *pool1, const int64_t *off1, const int32_t *len1,
                              const char *pool2, const int64_t *off2, const int32_t *len2, char *ops, const int64_t *ops_off, int32_t *ops_len)
{
	if (!c || n_pairs < 0) return GSA_ERR_ARG;
	if (n_pairs == 0) return GSA_OK;
	hipStream_t st = c->stream;
	const size_t n = (size_t)n_pairs;
	i64 p1 = 0, p2 = 0, po = 0;
	for (size_t i = 0; i < n; i++) {
		if (len1[i] < 0 || len2[i] < 0) return gsa_fail(c, GSA_ERR_ARG, "negative fragment length");
		if (off1[i] + len1[i] > p1) p1 = off1[i] + len1[i];
		if (off2[i] + len2[i] > p2) p2 = off2[i] + len2[i];
		if (ops_off[i] + len1[i] + len2[i] > po) po = ops_off[i] + len1[i] + len2[i];
	}
	uint8_t *d_p1 = dev_ensure<uint8_t>(c, c->leaf[0], (size_t)p1 + 1), *d_p2 = dev_ensure<uint8_t>(c, c->leaf[1], (size_t)p2 + 1), *d_ops = dev_ensure<uint8_t>(c, c->leaf[2], (size_t)po + 1);
	i64 *d_o1 = dev_ensure<i64>(c, c->leaf[3], n), *d_o2 = dev_ensure<i64>(c, c->leaf[4], n), *d_oo = dev_ensure<i64>(c, c->leaf[5], n);
	i32 *d_l1 = dev_ensure<i32>(c, c->leaf[6], n), *d_l2 = dev_ensure<i32>(c, c->leaf[7], n), *d_ol = dev_ensure<i32>(c, c->leaf[8], n);
	if (!d_p1 || !d_p2 || !d_ops || !d_o1 || !d_o2 || !d_oo || !d_l1 || !d_l2 || !d_ol) return GSA_ERR_NOMEM;
	GSA_CHECK(c, hipMemcpyAsync(d_p1, pool1, p1, hipMemcpyHostToDevice, st)); GSA_CHECK(c, hipMemcpyAsync(d_p2, pool2, p2, hipMemcpyHostToDevice, st));
	GSA_CHECK(c, hipMemcpyAsync(d_o1, off1, n * 8, hipMemcpyHostToDevice, st)); GSA_CHECK(c, hipMemcpyAsync(d_o2, off2, n * 8, hipMemcpyHostToDevice, st));
	GSA_CHECK(c, hipMemcpyAsync(d_oo, ops_off, n * 8, hipMemcpyHostToDevice, st));
	GSA_CHECK(c, hipMemcpyAsync(d_l1, len1, n * 4, hipMemcpyHostToDevice, st)); GSA_CHECK(c, hipMemcpyAsync(d_l2, len2, n * 4, hipMemcpyHostToDevice, st));
	const i32 cnts[2] = { n_pairs, (i32)po };
	GSA_CHECK(c, hipMemcpyAsync(c->d_mail.as<i32>() + M_NJOB, cnts, 8, hipMemcpyHostToDevice, st));      // M_NJOB, M_OPSTOT
	Ksw2Launch kl;
	int rc = run_ksw2_jobs(c, n_pairs, d_p1, d_o1, d_l1, d_p2, d_o2, d_l2, d_ops, d_oo, d_ol, po, &kl);
	if (rc == GSA_OK && kl.small_in_flight) GSA_CHECK(c, hipStreamWaitEvent(st, c->ev[12], 0));
	if (rc == GSA_OK) {
		i32 err = 0;
		GSA_CHECK(c, hipMemcpyAsync(ops, d_ops, po, hipMemcpyDeviceToHost, st));
		GSA_CHECK(c, hipMemcpyAsync(ops_len, d_ol, n * 4, hipMemcpyDeviceToHost, st));
		GSA_CHECK(c, hipMemcpyAsync(&err, c->d_mail.as<i32>() + M_DPERR2, 4, hipMemcpyDeviceToHost, st));
		GSA_CHECK(c, hipStreamSynchronize(st));
		if (err) { c->dp_dirty = c->dp_timeout = true; rc = gsa_fail(c, GSA_ERR_STATE, "internal: DP stripe hand-off timed out"); }
	}
	return rc;
}
