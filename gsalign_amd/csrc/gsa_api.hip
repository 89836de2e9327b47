// gsalign_amd/csrc/gsa_api.hip -- the C-ABI entry points (include/gsa_hip.h) that RUN a query and read its result; block lists: gsa_blocks.cpp
#include <algorithm>
#include <cstring>
#include "gsa_ctx.h"

void collect_events(gsa_ctx *c)
{
	if (!c->profiling && !c->prof_seed) { c->ev_pending = 0; return; }
	float ms;
	if ((c->ev_pending & 1) && !c->profiling) {      // (prof_seed: the seed kernel alone, summed over the contigs)
		if (hipEventElapsedTime(&ms, c->ev[0], c->ev[1]) == hipSuccess) {
			c->kernel_ms[0] = ms;
			c->acc_seed_ms += ms;
		}
	} else {
		if (c->ev_pending & 1) {
			if (hipEventElapsedTime(&ms, c->ev[0], c->ev[1]) == hipSuccess) c->kernel_ms[0] = ms;
			if (hipEventElapsedTime(&ms, c->ev[1], c->ev[2]) == hipSuccess) c->kernel_ms[1] = ms;
			if (hipEventElapsedTime(&ms, c->ev[2], c->ev[3]) == hipSuccess) c->kernel_ms[2] = ms;
		}
		if (c->ev_pending & 2) { if (hipEventElapsedTime(&ms, c->ev[4], c->ev[5]) == hipSuccess) c->kernel_ms[3] = ms; }
	}
	c->ev_pending = 0;
	(void)hipGetLastError();
}

// Back to the end of stage 1 of a contig whose hits were imported (gsa_finish_contig's retry): everything later is dropped, stages 2-8 run again from the hits
// this context still holds -- d_key_a / d_val_a are read-only for stage 2; the PosDiff bitmap it consumed is set again from the keys.
static int rewind_to_hits(gsa_ctx *c)
{
	const i64 n_seeds = c->n_seeds; const i32 n_groups = c->n_groups;
	if (int rc = reset_run_state(c)) return rc;
	GSA_CHECK(c, hipStreamSynchronize(c->stream));
	c->n_seeds = n_seeds; c->n_groups = n_groups; c->counters[2] = c->counters[3] = (u64)n_seeds;
	c->stage = 1;
	return stage1_restore_pdbm(c);
}

// What the passes over a stage-8 result (k_variants.hip, k_cigar.hip, k_cs.hip, k_lift.hip, k_track.hip, k_segs.hip, k_proj.hip, k_regions.hip, k_qtrack.hip) ask of the context before they run; `who`: the export, for the messages;
// need: the pass reads the positions of gsa_lift_set / the window of gsa_track_set / paints into the accumulator of gsa_proj_open / reads the regions of gsa_regions_set /
// the query-side window of gsa_qtrack_set
enum { NEED_POSITIONS = 1, NEED_WINDOW = 2, NEED_ACC = 4, NEED_REGIONS = 8, NEED_QWINDOW = 16 };
static int result_pass_ready(gsa_ctx *c, int32_t k, const char *who, unsigned need = 0)
{
	const std::string w(who);
	if (c->stage != 8 || c->split) return gsa_fail(c, GSA_ERR_STATE, w + ": the context holds no finished (stage 8) result");
	// (the pass reads the contig's bases on the device: a prefetch into the slot that held them leaves another contig there)
	if (c->q_cur == -2) return gsa_fail(c, GSA_ERR_STATE, w + ": the contig's device copy was overwritten by a prefetch");
	if (k < 0 || k >= (c->bnd.n ? c->bnd.n : 1)) return gsa_fail(c, GSA_ERR_ARG, w + ": contig index out of range");
	if ((need & NEED_POSITIONS) && c->lift_n <= 0) return gsa_fail(c, GSA_ERR_STATE, w + ": no positions (gsa_lift_set first)");
	if ((need & NEED_WINDOW) && c->track_w <= 0) return gsa_fail(c, GSA_ERR_STATE, w + ": no window (gsa_track_set first)");
	if ((need & NEED_ACC) && !c->proj) return gsa_fail(c, GSA_ERR_STATE, w + ": no accumulator (gsa_proj_open first)");
	if ((need & NEED_REGIONS) && c->reg_n <= 0) return gsa_fail(c, GSA_ERR_STATE, w + ": no regions (gsa_regions_set first)");
	if ((need & NEED_QWINDOW) && c->qtrack_w <= 0) return gsa_fail(c, GSA_ERR_STATE, w + ": no window (gsa_qtrack_set first)");
	GSA_CHECK(c, hipSetDevice(c->device));
	return GSA_OK;
}
static int pass_timing(const gsa_ctx *c, Pass pass, double *ms_sum, int64_t *n_calls)
{
	if (!c || !ms_sum || !n_calls) return GSA_ERR_ARG;
	*ms_sum = c->pass_stat[pass].ms_sum; *n_calls = (int64_t)c->pass_stat[pass].calls;
	return GSA_OK;
}

// One export of a pass over the stage-8 result the context holds: the answer zeroed (an answer the pass may do without: out_optional), the preconditions, the pass itself
// (`run`, its driver in its k_*.hip) between two clock reads, its time and the call counted
template <class Out, class Run>
static int result_pass(gsa_ctx *c, int32_t k, const char *who, unsigned need, Pass pass, Out *out, Run run, bool out_optional = false)
{
	if (!c || (!out && !out_optional)) return GSA_ERR_ARG;
	if (out) *out = Out();
	if (const int rc = result_pass_ready(c, k, who, need)) return rc;
	const auto t0 = std::chrono::steady_clock::now();
	const int rc = run();
	c->pass_stat[pass].ms_sum += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); c->pass_stat[pass].calls++;
	return rc;
}

// (cig: the CIGARs the cs pass computed on its way, for gsa_align_many_ex -- they lie in the CIGAR pass's own buffers; cig / have of the segs pass: as block_segs)
int cs_call(gsa_ctx *c, int32_t k, gsa_cs *out, gsa_cigars *cig) { return result_pass(c, k, "gsa_block_cs", 0, PASS_CS, out, [&] { return block_cs(c, k, out, cig); }); }
int lift_call(gsa_ctx *c, int32_t k, gsa_lifts *out) { return result_pass(c, k, "gsa_lift", NEED_POSITIONS, PASS_LIFT, out, [&] { return lift_positions(c, k, out); }); }
int regions_call(gsa_ctx *c, int32_t k, gsa_region_lifts *out) { return result_pass(c, k, "gsa_lift_regions", NEED_REGIONS, PASS_REG, out, [&] { return lift_regions(c, k, out); }); }
int track_call(gsa_ctx *c, int32_t k, gsa_tracks *out) { return result_pass(c, k, "gsa_ref_track", NEED_WINDOW, PASS_TRACK, out, [&] { return ref_track(c, k, out); }); }
int qtrack_call(gsa_ctx *c, int32_t k, gsa_qtracks *out) { return result_pass(c, k, "gsa_query_track", NEED_QWINDOW, PASS_QTRACK, out, [&] { return query_track(c, k, out); }); }
int segs_call(gsa_ctx *c, int32_t k, gsa_segs *out, gsa_cigars *cig, const gsa_cigars *have)
{
	if (c && out && cig) *cig = gsa_cigars();
	return result_pass(c, k, "gsa_block_segs", 0, PASS_SEG, out, [&] { return block_segs(c, k, out, cig, have); });
}
int proj_call(gsa_ctx *c, int32_t k, gsa_proj_stat *out) { return result_pass(c, k, "gsa_project", NEED_ACC, PASS_PROJ, out, [&] { return project_blocks(c, k, out); }, true); }

extern "C" {
// Back to stage 0 with the same contig: the query stays where gsa_set_query put it (device and host copy).
int gsa_rewind(gsa_ctx *c)
{
	if (!c) return GSA_ERR_ARG;
	if (c->qlen <= 0) return gsa_fail(c, GSA_ERR_STATE, "gsa_set_query first");
	if (c->q_cur == -2) return gsa_fail(c, GSA_ERR_STATE, "gsa_rewind: the contig's device copy was overwritten by a prefetch");
	GSA_CHECK(c, hipSetDevice(c->device));
	return reset_run_state(c);
}
int gsa_run_to(gsa_ctx *c, int stage)
{
	if (!c || stage < 0 || stage > 8) return GSA_ERR_ARG;
	if (c->bnd.n && stage < 8 && !c->bundle_call) return gsa_fail(c, GSA_ERR_STATE, "gsa_run_to: the context holds a bundle (gsa_align_bundle runs it); gsa_set_query first");
	// (between gsa_seed_chunks and gsa_finish_contig the context holds the hits of a chunk range only: stage 1 here would seed
	//  that range again and call the result a contig)
	if (c->split) return gsa_fail(c, GSA_ERR_STATE, "gsa_run_to: a split contig is finished with gsa_finish_contig");
	GSA_CHECK(c, hipSetDevice(c->device));
	int rc = GSA_OK;
	auto t_prev = std::chrono::steady_clock::now();
	while (c->stage < stage && rc == GSA_OK) {
		const int next = c->stage + 1;
		switch (next) {
		case 1: rc = stage1_seed(c); break;
		case 2: rc = stage2_chain(c); break;
		case 3: rc = stage345_refine(c); if (rc == GSA_OK && c->bnd.n) bundle_split_lists(c); break;      // device part of S3..S5, host list = S3 state
		case 4: case 5: case 6: rc = host_stage4_5_6(c, next); break;
		case 7: if (c->bnd.n) bundle_join_lists(c); rc = stage7_fill(c); break;
		case 8: rc = stage78_extend(c); if (rc == GSA_OK) rc = host_stage8_finish(c); break;
		}
		if (rc == GSA_OK) { c->stage = next; c->frags_stage = (next == 8) ? 8 : 0; }
		{ const auto t_now = std::chrono::steady_clock::now(); c->wall_ms[next] += std::chrono::duration<double, std::milli>(t_now - t_prev).count(); t_prev = t_now; }
	}
	if (stage == 8) c->wall_n++;
	if (const unsigned long long ov = gsa_take_grid_overflow()) rc = gsa_fail(c, GSA_ERR_LIMIT, "a kernel launch of " + std::to_string(ov) + " work-items (>= 2^32) was needed: contig too large for this build");
	// stages 1-2 leave work in flight (no count read-backs); the call returns with the stream idle
	if (rc == GSA_OK) { GSA_CHECK(c, hipStreamSynchronize(c->stream)); collect_events(c); }
	if (c->early_in_flight && (rc != GSA_OK || !c->early_consumed)) GSA_CHECK(c, hipStreamSynchronize(c->stream_aux[0]));      // a stage view (or an error) must not leave the early DP launch running
	return rc;
}

// To stage 8 and the blocks.  A stripe of the DP that waited longer than its bound for its predecessor (never observed with ticket-ordered stripes; kept as a
// safety net): `rewind`, then the stages again with one DP job per launch -- all stripes of a job are resident then.
static int run_to_end_with_retry(gsa_ctx *c, int (*rewind)(gsa_ctx *), gsa_result *out)
{
	c->dp_timeout = false;
	int rc = gsa_run_to(c, 8);
	if (rc == GSA_ERR_STATE && c->dp_timeout && !c->dp_safe) {
		c->dp_timeout = false; c->dp_safe = true;
		rc = rewind(c);
		if (rc == GSA_OK) rc = gsa_run_to(c, 8);
		c->dp_safe = false;
	}
	return rc ? rc : gsa_get_blocks(c, out);
}
int gsa_align_contig(gsa_ctx *c, const char *query, int32_t qlen, gsa_result *out)
{
	if (!c || !out) return GSA_ERR_ARG;
	if (int rc = gsa_set_query(c, query, qlen)) return rc;
	return run_to_end_with_retry(c, gsa_rewind, out);
}
int gsa_align_contig_device(gsa_ctx *c, const char *d_query, int32_t qlen, gsa_result *out)
{
	if (!c || !out) return GSA_ERR_ARG;
	if (int rc = gsa_set_query_device(c, d_query, qlen)) return rc;
	return run_to_end_with_retry(c, gsa_rewind, out);
}

// the result of contig k of the bundle this context just aligned (valid until the next call on the context)
static void bundle_result(gsa_ctx *c, int k, const std::vector<i64> &a0, size_t blk_at, gsa_result *out)
{
	out->n_blocks = c->b_nblk[(size_t)k]; out->blocks = c->h_blocks.data() + blk_at;
	out->n_frags = c->b_frag0[(size_t)k + 1] - c->b_frag0[(size_t)k]; out->recs = c->p_frags.as<gsa_rec>() + c->b_frag0[(size_t)k];
	out->n_aln = a0[(size_t)k + 1] - a0[(size_t)k]; out->aln1 = c->h_taln1 + a0[(size_t)k]; out->aln2 = c->h_taln2 + a0[(size_t)k];
}

// ---- several contigs in one pass (Bundle, gsa_internal.h; the concatenation and its tables: set_query_bundle, gsa_query.hip) ----
int gsa_align_bundle(gsa_ctx *c, const char *const *query, const int32_t *qlen, int32_t n, uint32_t flags, gsa_result *out)
{
	if (!c || !query || !qlen || !out || (flags & ~(uint32_t)GSA_MANY_DEVICE)) return GSA_ERR_ARG;
	int rc = set_query_bundle(c, query, qlen, n, (flags & GSA_MANY_DEVICE) != 0); if (rc) return rc;
	c->dp_timeout = false;
	c->bundle_call = true;
	struct Clear { gsa_ctx *c; ~Clear() { c->bundle_call = false; } } clear_{ c };
	rc = gsa_run_to(c, 8);
	if (rc == GSA_ERR_STATE && c->dp_timeout && !c->dp_safe) {      // (the safety net of gsa_align_contig; the concatenation stays where it is)
		c->dp_timeout = false; c->dp_safe = true;
		{ const Bundle keep = c->bnd; rc = reset_run_state(c); c->bnd = keep; }
		if (rc == GSA_OK) rc = gsa_run_to(c, 8);
		c->dp_safe = false;
	}
	if (rc) return rc;
	const size_t nfb = c->b_blk0.empty() ? 0 : (size_t)c->b_blk0[(size_t)n];
	if (nfb == 0 || c->n_frags == 0) {
		for (int k = 0; k < n; k++) { out[k].n_blocks = 0; out[k].n_frags = 0; out[k].n_aln = 0; out[k].blocks = nullptr; out[k].recs = nullptr; out[k].aln1 = out[k].aln2 = nullptr; }
		return GSA_OK;
	}
	// string-pool offset of every contig: k_bundle_rebase left it for the contigs that have records
	std::vector<i64> a0((size_t)n + 1, c->n_aln);
	for (int k = n - 1; k >= 0; k--) a0[(size_t)k] = c->b_blk0[(size_t)k] < c->b_blk0[(size_t)k + 1] ? c->p_ba0.as<i64>()[k] : a0[(size_t)k + 1];
	size_t at = 0;
	for (int k = 0; k < n; k++) { bundle_result(c, k, a0, at, &out[k]); at += (size_t)c->b_nblk[(size_t)k]; }
	return GSA_OK;
}

// ---- one contig seeded by several GPUs ----
int gsa_seed_chunks(gsa_ctx *c, const char *query, int32_t qlen, int32_t chunk_beg, int32_t chunk_end)
{
	if (!c || chunk_beg < 0 || chunk_end < chunk_beg) return GSA_ERR_ARG;
	int rc = gsa_set_query(c, query, qlen); if (rc) return rc;
	c->split = true; c->rng_beg = chunk_beg; c->rng_end = chunk_end;
	rc = stage1_seed(c);
	if (rc == GSA_OK) GSA_CHECK(c, hipStreamSynchronize(c->stream));
	collect_events(c);
	return rc;
}
int64_t gsa_hit_count(gsa_ctx *c) { return (c && c->split) ? c->n_seeds : 0; }
int gsa_export_hits(gsa_ctx *c, uint64_t *keys, uint32_t *vals)
{
	if (!c || !c->split) return c ? gsa_fail(c, GSA_ERR_STATE, "gsa_seed_chunks first") : GSA_ERR_ARG;
	if (c->n_seeds == 0) return GSA_OK;
	if (!keys || !vals) return GSA_ERR_ARG;
	GSA_CHECK(c, hipSetDevice(c->device));
	GSA_CHECK(c, hipMemcpyAsync(keys, c->d_key_a.p, (size_t)c->n_seeds * 8, hipMemcpyDefault, c->stream));
	GSA_CHECK(c, hipMemcpyAsync(vals, c->d_val_a.p, (size_t)c->n_seeds * 4, hipMemcpyDefault, c->stream));
	GSA_CHECK(c, hipStreamSynchronize(c->stream));
	return GSA_OK;
}
int gsa_import_hits(gsa_ctx *c, const uint64_t *keys, const uint32_t *vals, int64_t n)
{
	if (!c || n < 0 || (n > 0 && (!keys || !vals))) return GSA_ERR_ARG;
	if (!c->split || c->stage != 0) return gsa_fail(c, GSA_ERR_STATE, "gsa_seed_chunks first");
	GSA_CHECK(c, hipSetDevice(c->device));
	return stage1_import_hits(c, (const u64 *)keys, (const u32 *)vals, n);
}
int gsa_finish_contig(gsa_ctx *c, gsa_result *out)
{
	if (!c || !out) return GSA_ERR_ARG;
	if (!c->split || c->stage != 0) return gsa_fail(c, GSA_ERR_STATE, "gsa_seed_chunks first");
	GSA_CHECK(c, hipSetDevice(c->device));
	int rc = stage1_finish_split(c); if (rc) return rc;
	c->stage = 1; c->split = false;
	return run_to_end_with_retry(c, rewind_to_hits, out);
}

// The hits of this context's chunk range where they lie (device memory; valid until the next call on this context): what an
// owner on the same node imports directly -- gsa_import_hits(owner, keys, vals, n) copies device to device, peer to peer when the
// two contexts sit on different GPUs.
int gsa_hit_buffers(gsa_ctx *c, const uint64_t **keys, const uint32_t **vals)
{
	if (!c || !keys || !vals) return GSA_ERR_ARG;
	if (!c->split) return gsa_fail(c, GSA_ERR_STATE, "gsa_seed_chunks first");
	*keys = c->d_key_a.as<uint64_t>(); *vals = c->d_val_a.as<uint32_t>();
	return GSA_OK;
}

// VariantIdentification (SeqVariant.cpp:12-119) over the stage-8 result the context holds: k_variants.hip
int gsa_call_variants(gsa_ctx *c, int32_t k, gsa_variants *out)
{
	if (!c || !out) return GSA_ERR_ARG;
	out->n = 0; out->v = nullptr; out->n_snv = out->n_ins = out->n_del = 0;
	const int rc = result_pass_ready(c, k, "gsa_call_variants");
	return rc ? rc : call_variants(c, k, out);
}
int gsa_get_variant_timing(gsa_ctx *c, double *ms_sum, int64_t *n_calls) { return pass_timing(c, PASS_VAR, ms_sum, n_calls); }

// the CIGAR of every block of the stage-8 result the context holds: k_cigar.hip
int gsa_block_cigars(gsa_ctx *c, int32_t k, gsa_cigars *out) { return result_pass(c, k, "gsa_block_cigars", 0, PASS_CIG, out, [&] { return block_cigars(c, k, out); }); }
int gsa_get_cigar_timing(gsa_ctx *c, double *ms_sum, int64_t *n_calls) { return pass_timing(c, PASS_CIG, ms_sum, n_calls); }

int gsa_block_cs(gsa_ctx *c, int32_t k, gsa_cs *out) { return cs_call(c, k, out, nullptr); }
int gsa_get_cs_timing(gsa_ctx *c, double *ms_sum, int64_t *n_calls) { return pass_timing(c, PASS_CS, ms_sum, n_calls); }

int gsa_lift_set(gsa_ctx *c, const int64_t *pos, int64_t n)
{
	if (!c || n < 0 || (n > 0 && !pos)) return GSA_ERR_ARG;
	if (n >= (1ll << 31) - 256) return gsa_fail(c, GSA_ERR_LIMIT, "gsa_lift_set: too many positions");
	for (int64_t i = 0; i < n; i++) if (pos[i] < 0 || pos[i] >= c->G)
		return gsa_fail(c, GSA_ERR_ARG, "gsa_lift_set: position " + std::to_string((long long)pos[i]) + " (entry " + std::to_string((long long)i) + ") lies outside the reference [0, " + std::to_string((long long)c->G) + ")");
	if (n == 0) { c->lift_n = 0; return GSA_OK; }
	GSA_CHECK(c, hipSetDevice(c->device));
	// (the API is synchronous: no pass of this context reads the old positions any more)
	c->lift_n = 0;      // (a failed allocation or copy leaves the context without positions, never with half of them)
	ENS(i64, d_lpos, (size_t)n);
	const hipError_t e = hipMemcpy(c->d_lpos.p, pos, (size_t)n * sizeof(i64), hipMemcpyHostToDevice);
	if (e != hipSuccess) { return gsa_fail(c, GSA_ERR_HIP, std::string("gsa_lift_set (hipMemcpy H2D): ") + hipGetErrorString(e)); }
	c->lift_n = n;
	return GSA_OK;
}
int gsa_lift(gsa_ctx *c, int32_t k, gsa_lifts *out) { return lift_call(c, k, out); }
int gsa_get_lift_timing(gsa_ctx *c, double *ms_sum, int64_t *n_calls) { return pass_timing(c, PASS_LIFT, ms_sum, n_calls); }

int gsa_regions_set(gsa_ctx *c, const int64_t *beg, const int64_t *end, int64_t n)
{
	if (!c || n < 0 || (n > 0 && (!beg || !end))) return GSA_ERR_ARG;
	if (n >= (1ll << 31) - 256) return gsa_fail(c, GSA_ERR_LIMIT, "gsa_regions_set: too many regions");
	for (int64_t i = 0; i < n; i++) {
		const std::string who = "gsa_regions_set: region [" + std::to_string((long long)beg[i]) + ", " + std::to_string((long long)end[i]) + ") (entry " + std::to_string((long long)i) + ")";
		if (beg[i] < 0 || end[i] > c->G || beg[i] >= c->G) return gsa_fail(c, GSA_ERR_ARG, who + " lies outside the reference [0, " + std::to_string((long long)c->G) + ")");
		if (beg[i] >= end[i]) return gsa_fail(c, GSA_ERR_ARG, who + (beg[i] == end[i] ? " is empty" : " is reversed"));
		// (the sequence that holds beg: the last one that starts at or before it)
		const size_t s = (size_t)(std::upper_bound(c->h_chr_fwd.begin(), c->h_chr_fwd.end(), (i64)beg[i]) - c->h_chr_fwd.begin()) - 1;
		if (s >= c->h_chr_len.size() || end[i] > c->h_chr_fwd[s] + (i64)c->h_chr_len[s]) return gsa_fail(c, GSA_ERR_ARG, who + " crosses a sequence boundary");
	}
	if (n == 0) { c->reg_n = 0; return GSA_OK; }
	GSA_CHECK(c, hipSetDevice(c->device));
	// (the API is synchronous: no pass of this context reads the old regions any more)
	c->reg_n = 0;      // (a failed allocation or copy leaves the context without regions, never with half of them)
	ENS(i64, d_rgpos, 2 * (size_t)n);
	hipError_t e = hipMemcpy(c->d_rgpos.p, beg, (size_t)n * sizeof(i64), hipMemcpyHostToDevice);
	if (e == hipSuccess) e = hipMemcpy(c->d_rgpos.as<i64>() + n, end, (size_t)n * sizeof(i64), hipMemcpyHostToDevice);
	if (e != hipSuccess) { return gsa_fail(c, GSA_ERR_HIP, std::string("gsa_regions_set (hipMemcpy H2D): ") + hipGetErrorString(e)); }
	c->reg_n = n;
	return GSA_OK;
}
int gsa_lift_regions(gsa_ctx *c, int32_t k, gsa_region_lifts *out) { return regions_call(c, k, out); }
int gsa_get_region_timing(gsa_ctx *c, double *ms_sum, int64_t *n_calls) { return pass_timing(c, PASS_REG, ms_sum, n_calls); }

int gsa_track_set(gsa_ctx *c, int32_t window)
{
	if (!c) return GSA_ERR_ARG;
	if (window < 0) return gsa_fail(c, GSA_ERR_ARG, "gsa_track_set: the window is negative");
	i64 nwin = 0;
	if (window > 0) for (size_t i = 0; i < c->h_chr_len.size(); i++) nwin += ((i64)c->h_chr_len[i] + window - 1) / window;
	if (nwin >= (1ll << 31) - 256) return gsa_fail(c, GSA_ERR_LIMIT, "gsa_track_set: " + std::to_string((long long)nwin) + " windows (2^31 - 256 or more)");
	// (the dense counts are all zero between calls, whatever the window was: a new length only lays them out anew)
	c->track_w = window; c->track_nwin = nwin;
	return GSA_OK;
}
int gsa_ref_track(gsa_ctx *c, int32_t k, gsa_tracks *out) { return track_call(c, k, out); }
int gsa_get_track_timing(gsa_ctx *c, double *ms_sum, int64_t *n_calls) { return pass_timing(c, PASS_TRACK, ms_sum, n_calls); }
int gsa_qtrack_set(gsa_ctx *c, int32_t window)
{
	if (!c) return GSA_ERR_ARG;
	if (window < 0) return gsa_fail(c, GSA_ERR_ARG, "gsa_qtrack_set: the window is negative");
	c->qtrack_w = window;      // (the windows of a contig are fewer than its bases: no limit to check here; the dense array stays, all zero, whatever the window)
	return GSA_OK;
}
int gsa_query_track(gsa_ctx *c, int32_t k, gsa_qtracks *out) { return qtrack_call(c, k, out); }
int gsa_get_qtrack_timing(gsa_ctx *c, double *ms_sum, int64_t *n_calls) { return pass_timing(c, PASS_QTRACK, ms_sum, n_calls); }

int gsa_block_segs(gsa_ctx *c, int32_t k, gsa_segs *out) { return segs_call(c, k, out, nullptr, nullptr); }
int gsa_get_seg_timing(gsa_ctx *c, double *ms_sum, int64_t *n_calls) { return pass_timing(c, PASS_SEG, ms_sum, n_calls); }

int gsa_proj_open(gsa_ctx *c, gsa_ctx *share, uint32_t flags) { return c ? proj_open(c, share, flags) : GSA_ERR_ARG; }
int gsa_proj_close(gsa_ctx *c)
{
	if (!c) return GSA_ERR_ARG;
	if (!c->proj) return gsa_fail(c, GSA_ERR_STATE, "gsa_proj_close: no accumulator (gsa_proj_open first)");
	return proj_release(c);
}
int gsa_proj_clear(gsa_ctx *c)
{
	if (!c) return GSA_ERR_ARG;
	if (!c->proj) return gsa_fail(c, GSA_ERR_STATE, "gsa_proj_clear: no accumulator (gsa_proj_open first)");
	return proj_clear(c);
}
int gsa_project(gsa_ctx *c, int32_t k, gsa_proj_stat *out) { return proj_call(c, k, out); }
// (the two range calls share their checks; `who` for the messages)
static int proj_range_ready(gsa_ctx *c, int64_t p0, int64_t n, const char *who)
{
	if (!c) return GSA_ERR_ARG;
	if (!c->proj) return gsa_fail(c, GSA_ERR_STATE, std::string(who) + ": no accumulator (gsa_proj_open first)");
	if (n < 0 || p0 < 0 || p0 > c->proj->G || n > c->proj->G - p0) return gsa_fail(c, GSA_ERR_ARG, std::string(who) + ": the range lies outside the reference [0, " + std::to_string((long long)c->proj->G) + ")");
	return GSA_OK;
}
int gsa_proj_fetch(gsa_ctx *c, int64_t p0, int64_t n, char *text, uint32_t *words)
{
	if (const int rc = proj_range_ready(c, p0, n, "gsa_proj_fetch")) return rc;
	return (n == 0 || (!text && !words)) ? GSA_OK : proj_fetch(c, p0, n, text, words);
}
int gsa_proj_merge(gsa_ctx *c, int64_t p0, int64_t n, const uint32_t *words)
{
	if (const int rc = proj_range_ready(c, p0, n, "gsa_proj_merge")) return rc;
	if (n == 0) return GSA_OK;
	return words ? proj_merge(c, p0, n, words) : GSA_ERR_ARG;
}
int gsa_get_proj_timing(gsa_ctx *c, double *ms_sum, int64_t *n_calls) { return pass_timing(c, PASS_PROJ, ms_sum, n_calls); }

int gsa_get_wall_sums(gsa_ctx *c, double ms[10], int64_t *n)
{
	if (!c || !ms || !n) return GSA_ERR_ARG;
	memcpy(ms, c->wall_ms, sizeof(c->wall_ms)); *n = c->wall_n;
	if (c->up && c->own_up) { std::lock_guard<std::mutex> g(c->up->mu); ms[9] = c->up->jobs ? c->up->copy_ms / (double)c->up->jobs * (double)c->wall_n : 0.0; }      // (x n: the caller divides by n)
	return GSA_OK;
}
int gsa_get_alloc_stats(gsa_ctx *c, double *ms, int64_t *n, int64_t *bytes)
{
	if (!c) return GSA_ERR_ARG;
	if (ms) *ms = c->alloc_ms; if (n) *n = c->alloc_n; if (bytes) *bytes = c->alloc_bytes;
	return GSA_OK;
}

// enable: bit 0 stage timers and counters, bit 1 the accounting build of the seed kernel, bit 2 the seed kernel's time alone, bit 3 the variant passes' device time; every sum starts again
int gsa_set_profiling(gsa_ctx *c, int enable)
{
	if (!c) return GSA_ERR_ARG;
	c->acc_seed_ms = 0.0;
	memset(c->wall_ms, 0, sizeof(c->wall_ms));
	c->wall_n = 0;
	if (c->up && c->own_up) {
		std::lock_guard<std::mutex> g(c->up->mu);
		c->up->copy_ms = c->up->wait_ms = c->up->bytes = 0;
		c->up->jobs = 0;
	}
	c->pass_stat[PASS_VAR] = PassStat();
	c->prof_var = (enable & 8) != 0;
	c->profiling = (enable & 1) != 0;
	c->count_blocks = (enable & 2) != 0;
	c->prof_seed = (enable & 4) != 0;
	return GSA_OK;
}

int64_t gsa_seed_count(gsa_ctx *c) { return c ? c->n_seeds : 0; }
int gsa_get_seeds(gsa_ctx *c, gsa_seed *out)
{
	if (!c || (!out && c->n_seeds)) return GSA_ERR_ARG;
	if (c->stage < 1) return gsa_fail(c, GSA_ERR_STATE, "run stage 1 first");
	const size_t n = (size_t)c->n_seeds; if (!n) return GSA_OK;
	{ int rc = seed_view_sort(c); if (rc) return rc; GSA_CHECK(c, hipStreamSynchronize(c->stream)); }
	std::vector<i32> q(n), l(n); std::vector<i64> r(n);
	GSA_CHECK(c, hipMemcpy(q.data(), c->s_q.p, n * 4, hipMemcpyDeviceToHost));
	GSA_CHECK(c, hipMemcpy(l.data(), c->s_len.p, n * 4, hipMemcpyDeviceToHost));
	GSA_CHECK(c, hipMemcpy(r.data(), c->s_r.p, n * 8, hipMemcpyDeviceToHost));
	for (size_t i = 0; i < n; i++) { out[i].qpos = q[i]; out[i].len = l[i]; out[i].rpos = r[i]; }
	return GSA_OK;
}
int gsa_group_count(gsa_ctx *c)
{
	if (!c) return 0;
	if (c->n_groups < 0) {      // stage 1 leaves the count on the device
		if (seed_view_sort(c) != GSA_OK) return 0;
		hipStreamSynchronize(c->stream);
		i32 ng = 0;
		if (hipMemcpy(&ng, c->d_mail.as<i32>() + M_NG, 4, hipMemcpyDeviceToHost) != hipSuccess) return 0;
		c->n_groups = ng;
	}
	return c->n_groups;
}
int gsa_get_groups(gsa_ctx *c, int32_t *beg, int32_t *end)
{
	if (!c) return GSA_ERR_ARG;
	if (c->stage < 1) return gsa_fail(c, GSA_ERR_STATE, "run stage 1 first");
	const size_t ng = (size_t)gsa_group_count(c); if (!ng) return GSA_OK;
	std::vector<i32> gb(ng + 1);
	GSA_CHECK(c, hipMemcpy(gb.data(), c->g_beg.p, (ng + 1) * 4, hipMemcpyDeviceToHost));
	for (size_t i = 0; i < ng; i++) { beg[i] = gb[i]; end[i] = gb[i + 1]; }
	return GSA_OK;
}
int gsa_get_blocks(gsa_ctx *c, gsa_result *out)
{
	if (!c || !out) return GSA_ERR_ARG;
	if (c->stage < 2) return gsa_fail(c, GSA_ERR_STATE, "run stage 2 first");
	if (c->bnd.n && c->stage < 8) return gsa_fail(c, GSA_ERR_STATE, "gsa_get_blocks: the context holds a bundle -- only its finished result (gsa_align_bundle's out[]) is defined per contig");
	if (c->frags_stage != c->stage) { int rc = build_block_view(c); if (rc) return rc; }
	out->n_blocks = (int32_t)c->h_blocks.size(); out->blocks = c->h_blocks.data();
	if (c->result_pinned && c->stage == 8) {
		out->n_frags = c->n_frags; out->n_aln = c->n_aln;
		out->recs = c->p_frags.as<gsa_rec>(); out->aln1 = c->h_taln1; out->aln2 = c->h_taln2;
	} else {
		out->n_frags = (int64_t)c->h_frags.size(); out->n_aln = (int64_t)c->h_aln1.size();
		out->recs = c->h_frags.data(); out->aln1 = c->h_aln1.data(); out->aln2 = c->h_aln2.data();
	}
	return GSA_OK;
}
int gsa_get_counters(gsa_ctx *c, uint64_t counters[8]) { if (!c) return GSA_ERR_ARG; memcpy(counters, c->counters, sizeof(c->counters)); return GSA_OK; }
int gsa_get_timings(gsa_ctx *c, float ms[8]) { if (!c) return GSA_ERR_ARG; memcpy(ms, c->kernel_ms, sizeof(c->kernel_ms)); if (c->prof_seed && !c->profiling) ms[6] = (float)c->acc_seed_ms; return GSA_OK; }
int gsa_get_dp_stats(gsa_ctx *c, uint64_t st[4]) { if (!c) return GSA_ERR_ARG; memcpy(st, c->dp_stats, sizeof(c->dp_stats)); return GSA_OK; }
int gsa_get_seed_stats(gsa_ctx *c, uint64_t st[8]) { if (!c) return GSA_ERR_ARG; memcpy(st, c->dbg, sizeof(c->dbg)); return GSA_OK; }
// The counters that are never reset, and the two device ticket words held against their host twins: a fused pass (a sliced chain walk) numbers its tiles
// (slices) `device ticket - host value`, so one draw of difference makes every workgroup of the next launch wait out its bound for a tile that nobody holds.
int gsa_get_launch_counters(gsa_ctx *c, uint64_t v[8])
{
	if (!c || !v) return GSA_ERR_ARG;
	GSA_CHECK(c, hipSetDevice(c->device));
	ctx_quiesce(c);
	u32 lb_dev = 0, walk_dev = 0; uint64_t slices = 0;
	GSA_CHECK(c, hipMemcpy(&lb_dev, c->d_mail.as<u32>() + M_TICKET, 4, hipMemcpyDeviceToHost));
	if (c->w_j0.p) {
		std::vector<unsigned long long> w(c->w_j0.cap / 8);
		GSA_CHECK(c, hipMemcpy(w.data(), c->w_j0.p, w.size() * 8, hipMemcpyDeviceToHost));
		walk_dev = (u32)w[0];
		// (entry words: from word 4 on, one per slice; slice 0 has none)
		if (c->walk_last_epoch) { slices = 1; for (size_t k = 5; k < w.size(); k++) slices += (u32)(w[k] >> 32) == c->walk_last_epoch; }
	}
	v[0] = c->lb_epoch; v[1] = c->lb_base; v[2] = c->dp_epoch; v[3] = c->band_epoch; v[4] = c->walk_epoch; v[5] = c->walk_ticket; v[6] = slices; v[7] = c->d_dp_bnd.cap;
	if (lb_dev != c->lb_base) return gsa_fail(c, GSA_ERR_STATE, "ticket drift: the fused passes' device ticket is " + std::to_string(lb_dev) + ", the host counts " + std::to_string(c->lb_base));
	if (c->w_j0.p && walk_dev != c->walk_ticket) return gsa_fail(c, GSA_ERR_STATE, "ticket drift: the chain walk's device ticket is " + std::to_string(walk_dev) + ", the host counts " + std::to_string(c->walk_ticket));
	return GSA_OK;
}
} // extern "C"
