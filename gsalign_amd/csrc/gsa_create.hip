// gsalign_amd/csrc/gsa_create.hip -- the life cycle of a context behind the C ABI (include/gsa_hip.h): constructors and gsa_destroy, the index reservation, parameters
// and options, memory helpers, the index builder's wrapper.  The text of gsa_last_error(NULL) is private to this file: gsa_fail(nullptr, ...) sets it.
#include <algorithm>
#include <atomic>
#include <cstring>
#include <pthread.h>
#include <sched.h>
#include "gsa_ctx.h"

static thread_local std::string g_create_error;
int gsa_fail(gsa_ctx *ctx, int code, const std::string &msg)
{
	if (ctx) ctx->err = msg; else g_create_error = msg;
	return code;
}

// a constructor gives up: `msg`, or else the text the context holds, becomes gsa_last_error(NULL)'s; the context goes with everything it owns so far
static int ctx_abandon(gsa_ctx *c, int rc, const std::string &msg = std::string())
{
	if (!msg.empty()) g_create_error = msg; else if (!c->err.empty()) g_create_error = c->err;
	gsa_destroy(c);
	return rc;
}

// what a constructor checks before it allocates anything (`who`: the export, for the message): the device ordinal, the GSA_CREATE_* flags
static int create_device_ok(const char *who, int device)
{
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return gsa_fail(nullptr, GSA_ERR_HIP, "no HIP device available (libgsa_hip.so has no CPU path)"); }
	if (device < 0 || device >= ndev) return gsa_fail(nullptr, GSA_ERR_ARG, std::string(who) + ": bad device ordinal");
	return GSA_OK;
}
static int create_flags_ok(const char *who, uint32_t flags, uint32_t extra = 0u)
{
	if (flags & ~(uint32_t)(GSA_CREATE_WIDE | GSA_CREATE_KMER_K(15) | GSA_CREATE_PRIO(3) | GSA_CREATE_REF_PAC | extra)) return gsa_fail(nullptr, GSA_ERR_ARG, std::string(who) + ": unknown flag");
	if (((flags >> 8) & 15u) == 1) return gsa_fail(nullptr, GSA_ERR_ARG, std::string(who) + ": GSA_CREATE_KMER_K takes 2 .. 15 (0: chosen by text length and free memory)");
	return GSA_OK;
}

// a new context, flags decoded, its device current (c->err: what hipSetDevice said, if it failed) with host waits that spin instead of sleeping: the pipeline has ~20 short count read-backs per contig
static gsa_ctx *ctx_new(int device, uint32_t flags)
{
	gsa_ctx *c = new gsa_ctx();
	c->device = device; c->force_wide = (flags & GSA_CREATE_WIDE) != 0; c->opt.kmer_k = (int)((flags >> 8) & 15u); c->prio_mode = (int)((flags >> 16) & 3u);
	const hipError_t e = hipSetDevice(device);
	if (e != hipSuccess) c->err = hipGetErrorString(e); else (void)hipSetDeviceFlags(hipDeviceScheduleSpin);
	(void)hipGetLastError();
	return c;
}

static int uploader_start(gsa_ctx *c)
{
	Uploader *u = new Uploader(); u->device = c->device;
	if (hipStreamCreateWithFlags(&u->st, hipStreamNonBlocking) != hipSuccess) { delete u; return gsa_fail(c, GSA_ERR_HIP, "hipStreamCreate (upload stream)"); }
	u->th = std::thread([u] { u->run(); });      // (Uploader::run, gsa_query.hip)
	c->up = u; c->own_up = true;
	return GSA_OK;
}
static void uploader_stop(gsa_ctx *c)
{
	if (!c->up || !c->own_up) { c->up = nullptr; return; }
	Uploader *u = c->up;
	{ std::lock_guard<std::mutex> g(u->mu); u->stop = true; }
	u->cv.notify_all();
	if (u->th.joinable()) u->th.join();
#ifdef GSA_EXPERIMENTS
	if (getenv("GSA_UP_STATS") && u->jobs) fprintf(stderr, "[uploader] %lld jobs, %.1f MB each, %.2f ms in the queue, %.2f ms copying (%.1f GB/s)\n", (long long)u->jobs, u->bytes / 1e6 / u->jobs, u->wait_ms / u->jobs, u->copy_ms / u->jobs, u->bytes / 1e6 / u->copy_ms);
#endif
	if (u->st) hipStreamDestroy(u->st);
	delete u; c->up = nullptr;
}

// what every context owns, shared index or not: streams, events, counters, mailbox
static int ctx_private_init(gsa_ctx *c, gsa_ctx *share = nullptr)
{
	if (c->prio_mode > 0) {
		// GSA_CREATE_PRIO(mode): the MAIN stream -- the ~45 short passes of chaining / refinement / the extend stage's bookkeeping: little work, but every one of
		// them is a dispatch that has to find wave slots between the long kernels of the other contexts (measured with four contexts on the human index:
		// those phases take 6x their time alone, 11 of a contig's 19 ms: profiles/r05_contig_phases_human_full.txt) -- at the greatest priority; the seed-search
		// kernels move to a stream of their own (mode 1, 3: normal; mode 2: least) so that they do not inherit it; the striped DP's stream normal (mode 3: least)
		int lo = 0, hi = 0; GSA_CHECK(c, hipDeviceGetStreamPriorityRange(&lo, &hi));      // (lo = least, hi = greatest priority: numerically lo >= hi)
		const int mid = (lo + hi) / 2;
		GSA_CHECK(c, hipStreamCreateWithPriority(&c->stream, hipStreamDefault, hi));
		GSA_CHECK(c, hipStreamCreateWithPriority(&c->stream_seed, hipStreamDefault, c->prio_mode == 2 ? lo : mid));
		GSA_CHECK(c, hipEventCreateWithFlags(&c->ev_seed_fork, hipEventDisableTiming));
		for (int i = 0; i < 4; i++) GSA_CHECK(c, hipStreamCreateWithPriority(&c->stream_aux[i], hipStreamDefault, (c->prio_mode == 3 && (i == 0 || i == 3)) ? lo : mid));
	} else {
		GSA_CHECK(c, hipStreamCreate(&c->stream));
		for (int i = 0; i < 4; i++) GSA_CHECK(c, hipStreamCreate(&c->stream_aux[i]));
	}
	if (share) { c->up = share->up; c->own_up = false; } else if (int rc = uploader_start(c)) return rc;      // (Uploader, gsa_ctx.h)
	for (int i = 0; i < 28; i++) GSA_CHECK(c, hipEventCreate(&c->ev[i]));
	GSA_CHECK(c, hipMalloc(&c->d_zero.p, 256)); c->d_zero.cap = 256; GSA_CHECK(c, hipMemset(c->d_zero.p, 0, 256));      // (the bundle tables of a context that holds no bundle: bundle_off_flat)
	GSA_CHECK(c, hipMalloc(&c->d_cnt.p, 32 * sizeof(u64))); c->d_cnt.cap = 32 * sizeof(u64); GSA_CHECK(c, hipMemset(c->d_cnt.p, 0, 32 * sizeof(u64)));      // (16 counters + the seed kernel's ticket counter)
	GSA_CHECK(c, hipHostMalloc((void **)&c->h_cnt, 16 * sizeof(u64)));
	GSA_CHECK(c, hipMalloc(&c->d_mail.p, MAIL_N * sizeof(i32))); c->d_mail.cap = MAIL_N * sizeof(i32);
	GSA_CHECK(c, hipMemset(c->d_mail.p, 0, MAIL_N * sizeof(i32)));
	GSA_CHECK(c, hipHostMalloc((void **)&c->h_mail, MAIL_N * sizeof(i32)));
	return GSA_OK;
}

// One large index array, host to device.  Pageable memory goes through the runtime's staging buffers at ~12 GB/s; page-locked in place first (hipHostRegister:
// ~10 ms per GB) the copy is one DMA transfer at link speed -- 5.4 GB of a human index: 0.45 s -> 0.17 s.  A buffer that cannot be registered (already registered
// by the host, file-backed, too large for the limit) is copied as it is.
static hipError_t h2d_big(void *dst, const void *src, size_t bytes)
{
	if (bytes >= ((size_t)64 << 20) && hipHostRegister(const_cast<void *>(src), bytes, hipHostRegisterDefault) == hipSuccess) {
		const hipError_t e = hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice);
		(void)hipHostUnregister(const_cast<void *>(src));
		return e;
	}
	(void)hipGetLastError();
	return hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice);
}

// Device memory set aside for the two largest index tables before the index files are even read (gsa_reserve_index): their sizes follow from the text length
// alone.  One slot per device; gsa_create on that device adopts what fits (dev_take_reserved), gsa_release_reserved frees what was not used.
struct ReservedBuf { void *p = nullptr; size_t bytes = 0; };
static std::mutex g_res_mu; static ReservedBuf g_res[64][2];
void *dev_take_reserved(int device, size_t bytes, size_t *got)
{
	std::lock_guard<std::mutex> g(g_res_mu);
	for (int k = 0; k < 2; k++) { ReservedBuf &r = g_res[device & 63][k]; if (r.p && r.bytes >= bytes && r.bytes <= bytes + bytes / 8 + 4096) { void *p = r.p; *got = r.bytes; r.p = nullptr; r.bytes = 0; return p; } }
	return nullptr;
}

// the wide index builder (k_index_wide.hip): its bound, and the caps gsa_create_from_pac hands it (gsa_set_index_build_caps)
static const int64_t IX_WIDE_MAX_G = 4294967295ll;
static std::atomic<int64_t> g_ix_batch_cap{ 0 }, g_ix_occ_segment{ 0 }, g_ix_active_cap{ 0 };

// ChrLocMap (bwt_index.cpp:240-253) as a sorted table of last coordinates, host and device; the error text goes to gsa_last_error(NULL) (the caller destroys c)
static int ctx_chr_tables(gsa_ctx *c, const int32_t *chr_len, int32_t n_chr, i64 G, const char *who)
{
	c->G = G;
	i64 tot = 0; std::vector<std::pair<i64, i32> > ends;
	for (int i = 0; i < n_chr; i++) {
		c->h_chr_len.push_back(chr_len[i]); c->h_chr_fwd.push_back(tot); tot += chr_len[i];
		ends.push_back(std::make_pair(c->h_chr_fwd[i] + chr_len[i] - 1, i));
		ends.push_back(std::make_pair(2 * G - tot + chr_len[i] - 1, i));
	}
	if (tot != G) return gsa_fail(nullptr, GSA_ERR_ARG, std::string(who) + ": sum(chr_len) != G");
	std::sort(ends.begin(), ends.end());
	for (size_t i = 0; i < ends.size(); i++) { c->h_chr_end.push_back(ends[i].first); c->h_chr_of_end.push_back(ends[i].second); }
	c->d_chr_end.cap = c->h_chr_end.size() * 8; c->d_chr_of_end.cap = c->h_chr_of_end.size() * 4;
	hipError_t e = hipMalloc(&c->d_chr_end.p, c->h_chr_end.size() * 8);
	if (e == hipSuccess) e = hipMemcpy(c->d_chr_end.p, c->h_chr_end.data(), c->h_chr_end.size() * 8, hipMemcpyHostToDevice);
	if (e == hipSuccess) e = hipMalloc(&c->d_chr_of_end.p, c->h_chr_of_end.size() * 4);
	if (e == hipSuccess) e = hipMemcpy(c->d_chr_of_end.p, c->h_chr_of_end.data(), c->h_chr_of_end.size() * 4, hipMemcpyHostToDevice);
	if (e != hipSuccess) { (void)hipGetLastError(); return gsa_fail(nullptr, GSA_ERR_HIP, std::string(who) + ": chromosome tables: " + hipGetErrorString(e)); }
	c->di.chr_end = c->d_chr_end.as<i64>(); c->di.chr_of_end = c->d_chr_of_end.as<i32>(); c->di.n_ends = (i32)c->h_chr_end.size();
	return GSA_OK;
}

extern "C" {
void gsa_default_params(gsa_params *p)
{
	// main.cpp:202-214
	p->min_seed_len = 15; p->max_indel = 25; p->min_block_score = 200; p->min_aln_len = 200; p->min_identity = 70;
	p->sensitive = 0; p->one_on_one = 0;
}
const char *gsa_last_error(gsa_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }
int gsa_set_params(gsa_ctx *c, const gsa_params *p)
{
	if (!c || !p) return GSA_ERR_ARG;
	if (p->min_seed_len < 1 || p->max_indel < 0) return gsa_fail(c, GSA_ERR_ARG, "bad parameter");
	GSA_CHECK(c, hipSetDevice(c->device));
	// The presence bitmap and the short k-mer table depend on MinSeedLength and are read by every context cloned FROM this one
	// (gsa_clone copies the pointers): rebuilding them here -- in place, or freed and reallocated -- would hand those clones a
	// bitmap of another k or freed memory.  A clone that changes its own parameters builds tables of its own.
	if (c->n_borrowers.load() > 0 && (p->sensitive ? 10 : p->min_seed_len) != c->prm.MinSeedLength)
		return gsa_fail(c, GSA_ERR_STATE, "gsa_set_params: contexts cloned from this one read its seed tables -- change -slen / -sen on the clones, or destroy them first");
	if (int rc = reset_run_state(c)) return rc;
	c->prm.MinSeedLength = p->sensitive ? 10 : p->min_seed_len;         // main.cpp:323
	c->prm.MaxIndelSize = p->max_indel; c->prm.MinAlnBlockScore = p->min_block_score; c->prm.MinAlnLength = p->min_aln_len;
	c->prm.MinSeqIdy = p->min_identity; c->prm.bSensitive = p->sensitive ? 1 : 0; c->prm.OneOnOne = p->one_on_one ? 1 : 0;
	return build_presence(c);
}

int gsa_create(int device, const gsa_index_view *idx, const gsa_params *prm, gsa_ctx **out) { return gsa_create_opts(device, idx, prm, 0u, out); }
int gsa_create_opts(int device, const gsa_index_view *idx, const gsa_params *prm, uint32_t flags, gsa_ctx **out)
{
	if (!idx || !out || !idx->bwt || !idx->sa || !idx->ref || !idx->chr_len || idx->n_chr <= 0 || idx->G <= 0) return gsa_fail(nullptr, GSA_ERR_ARG, "gsa_create: bad index view");
	if (idx->L2[4] != (uint64_t)(2 * idx->G)) return gsa_fail(nullptr, GSA_ERR_ARG, "gsa_create: L2[4] != 2G");
	if (int rc = create_device_ok("gsa_create", device)) return rc;
	if (int rc = create_flags_ok("gsa_create_opts", flags)) return rc;
	gsa_ctx *c = ctx_new(device, flags);
#define CK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return ctx_abandon(c, GSA_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); } while (0)
	if (!c->err.empty()) return ctx_abandon(c, GSA_ERR_HIP, "hipSetDevice(device): " + c->err);
	if (int rc = ctx_private_init(c)) return ctx_abandon(c, rc);
	const size_t bwt_bytes = ((idx->bwt_words + 15) / 16) * 64;          // whole 64-byte blocks of the reference's layout (regrouped below: build_occ)
	CK(hipMalloc(&c->d_bwt_ref.p, bwt_bytes + 64)); c->d_bwt_ref.cap = bwt_bytes + 64;      // (freed once regrouped)
	CK(hipMemset(c->d_bwt_ref.p, 0, bwt_bytes + 64));
	CK(h2d_big(c->d_bwt_ref.p, idx->bwt, idx->bwt_words * 4));
	CK(hipMalloc(&c->d_sa.p, idx->n_sa * 8)); c->d_sa.cap = idx->n_sa * 8;
	CK(h2d_big(c->d_sa.p, idx->sa, idx->n_sa * 8));
	CK(hipMalloc(&c->d_ref.p, (size_t)2 * idx->G + 64)); c->d_ref.cap = (size_t)2 * idx->G + 64;
	if (flags & GSA_CREATE_REF_PAC) {
		// idx->ref = the .pac bytes (four bases per byte, first base in the top bits: bntseq.c's _get_pac): RestoreReferenceInfo's loop (bwt_index.cpp:229-264) runs
		// on the device -- G / 4 bytes cross PCIe instead of 2G, and the host need not have unpacked anything before the table builds start
		const size_t pac_bytes = ((size_t)idx->G + 3) / 4;
		void *d_pac = nullptr;
		CK(hipMalloc(&d_pac, pac_bytes + 64));
		if (h2d_big(d_pac, idx->ref, pac_bytes) != hipSuccess) { hipFree(d_pac); return ctx_abandon(c, GSA_ERR_HIP, "hipMemcpy (.pac)"); }
		const int rcu = unpack_pac(c, (const uint8_t *)d_pac, idx->G, (uint8_t *)c->d_ref.p);
		(void)hipStreamSynchronize(c->stream); hipFree(d_pac);
		if (rcu) return ctx_abandon(c, rcu);
	} else
	CK(h2d_big(c->d_ref.p, idx->ref, (size_t)2 * idx->G));
#undef CK
	if (int rc = ctx_chr_tables(c, idx->chr_len, idx->n_chr, idx->G, "gsa_create")) return ctx_abandon(c, rc);
	c->di.primary = idx->primary; for (int i = 0; i < 5; i++) c->di.L2[i] = idx->L2[i]; c->di.L2[0] = 0;
	c->di.seq_len = idx->L2[4];
	c->di.sa = c->d_sa.as<u64>(); c->di.ref = c->d_ref.as<uint8_t>(); c->di.G = idx->G;      // (the other tables: the builders below)
	{
		const int rco = build_occ(c, c->d_bwt_ref.p, bwt_bytes / 64);
		hipFree(c->d_bwt_ref.p); c->d_bwt_ref.p = nullptr; c->d_bwt_ref.cap = 0;
		if (rco) return ctx_abandon(c, rco);
	}
	if (int rc = build_dense_sa(c, idx->n_sa)) return ctx_abandon(c, rc);
	gsa_params dp; gsa_default_params(&dp);
	if (int rc = gsa_set_params(c, prm ? prm : &dp)) return ctx_abandon(c, rc);
	gsa_release_reserved(device);      // (a reservation that did not fit this index)
	if (const unsigned long long ov = gsa_take_grid_overflow()) return ctx_abandon(c, GSA_ERR_LIMIT, "gsa_create: a table build needed a launch of " + std::to_string(ov) + " work-items (>= 2^32)");
	*out = c;
	return GSA_OK;
}

// The context gsa_create_opts makes from the index files of a sequence, from the sequence itself: bwa_idx_build (bwtindex.c:77-149) and bwa_idx_load + RestoreReferenceInfo
// (bwt_index.cpp:147-264) in one pass over device memory.  The suffix sort of gsa_build_index runs on the new context's own stream; its SA array BECOMES the dense SA
// (k_densify_sa's LF walk is not launched), the file layout of the .bwt words lives in a device buffer only until build_occ has regrouped it, the SA samples are written where
// the context keeps them.  The remaining tables are built by the code gsa_create_opts runs (build_tables_from_pac, k_index.hip; build_ref2 / build_kmer_table, k_tables.hip).
int gsa_create_from_pac(int device, const uint8_t *pac, int64_t G, const int32_t *chr_len, int32_t n_chr, const gsa_params *prm, uint32_t flags, gsa_ctx **out)
{
	if (!pac || !chr_len || !out || G <= 0 || n_chr <= 0) return gsa_fail(nullptr, GSA_ERR_ARG, "gsa_create_from_pac: bad argument");
	{ int64_t tot = 0; for (int i = 0; i < n_chr; i++) { if (chr_len[i] <= 0) { tot = -1; break; } tot += chr_len[i]; } if (tot != G) return gsa_fail(nullptr, GSA_ERR_ARG, "gsa_create_from_pac: sum(chr_len) != G"); }
	if (int rc = create_flags_ok("gsa_create_from_pac", flags, GSA_CREATE_SORT_WIDE)) return rc;
	const bool sort_wide = (flags & GSA_CREATE_SORT_WIDE) != 0;
	if (sort_wide) flags |= GSA_CREATE_WIDE;      // (the 64-bit SA array is adopted as it is)
	// the bound of the device builder (gsa_build_index): 32-bit suffix indices; of the wide one (gsa_build_index_opts): a 33-bit rank in a sort key
	if (sort_wide && G > IX_WIDE_MAX_G) return gsa_fail(nullptr, GSA_ERR_LIMIT, "gsa_create_from_pac: the reference is longer than 4 294 967 295 bases (the wide device builder's sort key holds a 33-bit rank)");
	if (!sort_wide && 2 * G + 1 > (1ll << 31) - 2) return gsa_fail(nullptr, GSA_ERR_LIMIT, "gsa_create_from_pac: the reference is longer than 1 073 741 822 bases (the device builder sorts 32-bit suffix indices)");
	if (int rc = create_device_ok("gsa_create_from_pac", device)) return rc;
	gsa_ctx *c = ctx_new(device, flags);
	if (!c->err.empty()) return ctx_abandon(c, GSA_ERR_HIP, "gsa_create_from_pac: hipSetDevice");
	gsa_release_reserved(device);      // (a reservation is for the tables of gsa_create: the builder needs the room, and the dense SA is its own array)
	if (int rc = ctx_private_init(c)) return ctx_abandon(c, rc);
	if (hipMalloc(&c->d_ref.p, (size_t)2 * G + 64) != hipSuccess) { (void)hipGetLastError(); return ctx_abandon(c, GSA_ERR_NOMEM, "gsa_create_from_pac: hipMalloc (RefSequence)"); }
	c->d_ref.cap = (size_t)2 * G + 64;
	if (int rc = ctx_chr_tables(c, chr_len, n_chr, G, "gsa_create_from_pac")) return ctx_abandon(c, rc);
	c->di.ref = c->d_ref.as<uint8_t>(); c->di.G = G;      // (the other tables: the builders below)
	if (int rc = build_tables_from_pac(c, pac, G, IxOpts{ sort_wide, g_ix_batch_cap.load(), g_ix_occ_segment.load(), g_ix_active_cap.load() })) return ctx_abandon(c, rc);
	if (int rc = build_ref2(c)) return ctx_abandon(c, rc);
	if (int rc = build_kmer_table(c)) return ctx_abandon(c, rc);
	gsa_params dp; gsa_default_params(&dp);
	if (int rc = gsa_set_params(c, prm ? prm : &dp)) return ctx_abandon(c, rc);
	if (const unsigned long long ov = gsa_take_grid_overflow()) return ctx_abandon(c, GSA_ERR_LIMIT, "gsa_create_from_pac: a table build needed a launch of " + std::to_string(ov) + " work-items (>= 2^32)");
	*out = c;
	return GSA_OK;
}

// Test support: one device table of a context, as it lies in device memory, to the host -- its DEFINED extent, not the allocation's slack.
int gsa_export_index_table(gsa_ctx *c, int which, void *dst, uint64_t cap, uint64_t *bytes)
{
	if (!c || !bytes) return GSA_ERR_ARG;
	const DevIndex &di = c->di;
	uint64_t hdr[6] = { di.primary, di.L2[0], di.L2[1], di.L2[2], di.L2[3], di.L2[4] };
	uint64_t bw = 0, ns = 0;
	if (di.G <= 0 || gsa_index_sizes(di.G, &bw, &ns) != GSA_OK) return gsa_fail(c, GSA_ERR_STATE, "gsa_export_index_table: the context holds no index");
	const uint64_t n_blocks = 2 * ((bw + 15) / 16);      // build_occ: 64-row blocks, two uint4 each
	const void *src = nullptr; uint64_t n = 0; bool host = false;
	switch (which) {
	case GSA_TABLE_HEADER:   src = hdr; n = sizeof(hdr); host = true; break;
	case GSA_TABLE_OCC:      src = di.bwt; n = 2 * n_blocks * sizeof(uint4); break;
	case GSA_TABLE_OCC_BASE: src = di.occ_base; n = 4 * ((n_blocks >> di.occ_shift) + 1) * sizeof(u64); break;
	case GSA_TABLE_SA_DENSE: src = di.sa32 ? (const void *)di.sa32 : (const void *)di.sa64; n = (di.seq_len + 1) * (di.sa32 ? 4 : 8); break;
	case GSA_TABLE_SA:       src = di.sa; n = ns * 8; break;
	case GSA_TABLE_KMER:     src = di.kmer; n = ((uint64_t)(di.kmer_e16 ? 16 : 32)) << (2 * di.kmer_k); break;
	case GSA_TABLE_KMER_LO:  src = di.kmer_lo; n = ((uint64_t)(di.kmer_e16 ? 16 : 32)) << (2 * di.kmer_lo_k); break;
	case GSA_TABLE_PRES:     src = di.pres; n = di.pres_k >= 3 ? ((uint64_t)32 << (2 * (di.pres_k - 3))) : 0; break;
	case GSA_TABLE_REF:      src = di.ref; n = 2 * (uint64_t)di.G; break;
	case GSA_TABLE_REF2:     src = di.ref2; n = (di.seq_len / 16 + 8) * 4; break;
	default: return gsa_fail(c, GSA_ERR_ARG, "gsa_export_index_table: unknown table");
	}
	if (!src) n = 0;      // (an absent table)
	*bytes = n;
	if (!dst || n == 0) return GSA_OK;
	if (cap < n) return gsa_fail(c, GSA_ERR_ARG, "gsa_export_index_table: the buffer is too small");
	if (host) { memcpy(dst, src, n); return GSA_OK; }
	GSA_CHECK(c, hipSetDevice(c->device));
	GSA_CHECK(c, hipStreamSynchronize(c->stream));
	GSA_CHECK(c, hipMemcpy(dst, src, n, hipMemcpyDeviceToHost));
	return GSA_OK;
}

void gsa_destroy(gsa_ctx *c)
{
	if (!c) return;
	hipSetDevice(c->device);
	if (c->stream) hipStreamSynchronize(c->stream);
	for (int i = 0; i < 2; i++) slot_wait(c->qs[i]);
	uploader_stop(c);
	if (c->lender) c->lender->n_borrowers.fetch_sub(1);      // (`parent` outlives its clones: gsa_hip.h)
	(void)proj_release(c);      // (its reference to a projection accumulator, if it holds one: the last holder frees the array)
	// (a gsa_clone context borrows the index through `di` only: its index DevBufs are empty, a presence bitmap it built after
	//  a parameter change is its own)
#define X(n) if (c->n.p) hipFree(c->n.p);
	GSA_DEVBUFS(X)
#undef X
	if (c->h_cnt) hipHostFree(c->h_cnt);
	if (c->h_mail) hipHostFree(c->h_mail);
#define X(n) if (c->n.p) hipHostFree(c->n.p);
	GSA_PINBUFS(X)
#undef X
	for (int i = 0; i < 2; i++) if (c->ev_var[i]) hipEventDestroy(c->ev_var[i]);
	for (int i = 0; i < 28; i++) if (c->ev[i]) hipEventDestroy(c->ev[i]);
	for (int i = 0; i < 4; i++) if (c->stream_aux[i]) hipStreamDestroy(c->stream_aux[i]);
	if (c->stream_seed) hipStreamDestroy(c->stream_seed);
	if (c->ev_seed_fork) hipEventDestroy(c->ev_seed_fork);
	if (c->stream) hipStreamDestroy(c->stream);
	delete c;
}

// A second context on the same GPU that shares `parent`'s device-resident index (read-only: BWT + Occ, both SAs, k-mer
// table, packed and ASCII text, chromosome table) and owns everything else.  What the reference does with N pthreads
// on one contig, a host does here with N contexts on N contigs: while one contig sits in the dependency chain of its
// largest DP problem, the next one's seed search and chaining fill the idle CUs, and its upload overlaps both.
int gsa_clone(gsa_ctx *parent, gsa_ctx **out)
{
	if (!parent || !out) return GSA_ERR_ARG;
	if (hipSetDevice(parent->device) != hipSuccess) return gsa_fail(nullptr, GSA_ERR_HIP, "hipSetDevice");
	gsa_ctx *c = new gsa_ctx();
	c->device = parent->device; c->force_wide = parent->force_wide; c->prio_mode = parent->prio_mode;
	c->index_owner = parent->index_owner ? parent->index_owner : parent; c->seed_budget = parent->seed_budget; c->opt = parent->opt;
	if (int rc = ctx_private_init(c, c->index_owner)) return ctx_abandon(c, rc);
	c->di = parent->di; c->G = parent->G;
	c->lender = parent; parent->n_borrowers.fetch_add(1);
	c->h_chr_end = parent->h_chr_end; c->h_chr_fwd = parent->h_chr_fwd; c->h_chr_of_end = parent->h_chr_of_end; c->h_chr_len = parent->h_chr_len;
	c->prm = parent->prm;
	*out = c;
	return GSA_OK;
}

// A context on ANOTHER GPU (or the same one) with a device index of its own that is COPIED from `parent`'s, device to device, instead of uploaded
// and rebuilt: the Occ blocks, both suffix arrays, the k-mer tables, the presence table and both text forms are plain position-independent arrays, so a
// second GPU needs none of gsa_create's work -- the 10.7 GB over PCIe, the regrouping, the dense-SA walk, the table scans (1.3 - 2.7 s for the
// human index) -- only the bytes, over xGMI.  The host-side state being replicated is bwt_index.cpp:147-264's (RefIdx, RefSequence, ChrLocMap).
int gsa_clone_to_device(gsa_ctx *parent, int device, gsa_ctx **out)
{
	if (!parent || !out) return GSA_ERR_ARG;
	int ndev = 0;      // (not create_device_ok: one message and GSA_ERR_ARG whatever is wrong with the ordinal)
	if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) { (void)hipGetLastError(); return gsa_fail(nullptr, GSA_ERR_ARG, "gsa_clone_to_device: bad device ordinal"); }
	gsa_ctx *own = parent->index_owner ? parent->index_owner : parent;
	if (hipSetDevice(parent->device) != hipSuccess) return gsa_fail(nullptr, GSA_ERR_HIP, "hipSetDevice");
	if (hipStreamSynchronize(parent->stream) != hipSuccess || hipStreamSynchronize(own->stream) != hipSuccess) return gsa_fail(nullptr, GSA_ERR_HIP, "gsa_clone_to_device: the parent's stream");      // (tables a gsa_set_params has just queued)
	if (hipSetDevice(device) != hipSuccess) return gsa_fail(nullptr, GSA_ERR_HIP, "hipSetDevice");
	(void)hipSetDeviceFlags(hipDeviceScheduleSpin); (void)hipGetLastError();
	gsa_ctx *c = new gsa_ctx();
	c->device = device; c->force_wide = parent->force_wide; c->prio_mode = parent->prio_mode; c->seed_budget = parent->seed_budget; c->opt = parent->opt;
	if (int rc = ctx_private_init(c)) return ctx_abandon(c, rc);
	// every index table of the owner (and the tables a clone built for parameters of its own: presence bitmap, short k-mer table)
	struct Pair { const DevBuf *src; DevBuf *dst; };
	std::vector<Pair> tab = { { &own->d_bwt, &c->d_bwt }, { &own->d_occ_base, &c->d_occ_base }, { &own->d_sa, &c->d_sa }, { &own->d_ref, &c->d_ref }, { &own->d_chr_end, &c->d_chr_end },
		{ &own->d_chr_of_end, &c->d_chr_of_end }, { &own->d_sa_dense, &c->d_sa_dense }, { &own->d_kmer, &c->d_kmer }, { &own->d_ref2, &c->d_ref2 } };
	for (gsa_ctx *src = parent; src; src = src->lender) {      // (a clone reads these two through the context it was cloned from, unless it built its own)
		if (!c->d_pres.cap && src->d_pres.p && (const void *)parent->di.pres == src->d_pres.p) { tab.push_back({ &src->d_pres, &c->d_pres }); c->d_pres.cap = 1; }
		if (!c->d_kmer_lo.cap && src->d_kmer_lo.p && (const void *)parent->di.kmer_lo == src->d_kmer_lo.p) { tab.push_back({ &src->d_kmer_lo, &c->d_kmer_lo }); c->d_kmer_lo.cap = 1; }
	}
	c->d_pres.cap = c->d_kmer_lo.cap = 0;
	for (const Pair &t : tab) {
		if (!t.src->p) continue;
		const size_t bytes = t.src->len ? t.src->len : t.src->cap;
		if (bytes == 0) return ctx_abandon(c, GSA_ERR_STATE, "gsa_clone_to_device: an index table of unknown size");
		if (hipMalloc(&t.dst->p, bytes + 256) != hipSuccess) { (void)hipGetLastError(); return ctx_abandon(c, GSA_ERR_NOMEM, "gsa_clone_to_device: hipMalloc of an index table"); }
		t.dst->cap = bytes + 256; t.dst->len = bytes;
		const hipError_t e = (device == own->device) ? hipMemcpyAsync(t.dst->p, t.src->p, bytes, hipMemcpyDeviceToDevice, c->stream)
		                                             : hipMemcpyPeerAsync(t.dst->p, device, t.src->p, own->device, bytes, c->stream);
		if (e != hipSuccess) return ctx_abandon(c, GSA_ERR_HIP, std::string("gsa_clone_to_device: device-to-device copy: ") + hipGetErrorString(e));
	}
	// `di` with every pointer moved to the copy it points into
	c->di = parent->di;
	auto move_ptr = [&](const void *p) -> const void * {
		if (!p) return nullptr;
		for (const Pair &t : tab) if (t.src->p && (const char *)p >= (const char *)t.src->p && (const char *)p < (const char *)t.src->p + (t.src->len ? t.src->len : t.src->cap)) return (const char *)t.dst->p + ((const char *)p - (const char *)t.src->p);
		return (const void *)~(uintptr_t)0;
	};
	bool lost = false;
#define MOVE(field, T) do { const void *q_ = move_ptr((const void *)c->di.field); if (q_ == (const void *)~(uintptr_t)0) lost = true; c->di.field = (T)q_; } while (0)
	MOVE(bwt, const uint4 *); MOVE(occ_base, const u64 *); MOVE(sa, const u64 *); MOVE(sa32, const u32 *); MOVE(sa64, const u64 *); MOVE(ref, const uint8_t *); MOVE(ref2, const u32 *);
	MOVE(chr_end, const i64 *); MOVE(chr_of_end, const i32 *); MOVE(kmer, const u64 *); MOVE(kmer_lo, const u64 *); MOVE(pres, const u32 *);
#undef MOVE
	if (lost) return ctx_abandon(c, GSA_ERR_STATE, "gsa_clone_to_device: an index pointer outside the tables of its owner");
	c->G = parent->G;
	c->h_chr_end = parent->h_chr_end; c->h_chr_fwd = parent->h_chr_fwd; c->h_chr_of_end = parent->h_chr_of_end; c->h_chr_len = parent->h_chr_len;
	c->prm = parent->prm;
	if (hipStreamSynchronize(c->stream) != hipSuccess) return ctx_abandon(c, GSA_ERR_HIP, "gsa_clone_to_device: waiting for the copies");
	*out = c;
	return GSA_OK;
}

int gsa_reserve_index(int device, uint64_t seq_len, uint32_t flags)
{
	int ndev = 0;      // (not create_device_ok: this call leaves no message)
	if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev || seq_len == 0) { (void)hipGetLastError(); return GSA_ERR_ARG; }
	if (hipSetDevice(device) != hipSuccess) return GSA_ERR_HIP;
	const bool wide = (flags & GSA_CREATE_WIDE) != 0 || seq_len >= 0xFFFFFFF0ull;
	size_t want[2];
	want[0] = ((size_t)seq_len + 1 + 32) * (wide ? 8 : 4) + 256;                 // dense SA (build_dense_sa: rows + 32 entries, exact)
	{	// k-mer table: build_dense_sa's choice of k (text length, a quarter of the free memory, GSA_CREATE_KMER_K)
		int k = 0; while ((1ull << (2 * k)) < seq_len) k++;
		k += 2; if (k > 15) k = 15;
		size_t fr = 0, tot = 0; if (hipMemGetInfo(&fr, &tot) != hipSuccess) { (void)hipGetLastError(); fr = 8ull << 30; }
		const size_t esz = wide ? 32 : 16;
		while (k > 2 && ((size_t)esz << (2 * k)) > fr / 4) k--;
		const int kk = (int)((flags >> 8) & 15u); if (kk >= 2 && kk <= 15 && ((size_t)esz << (2 * kk)) <= fr / 2) k = kk;
		want[1] = k >= 2 ? ((size_t)esz << (2 * k)) : 0;
	}
	gsa_release_reserved(device);
	for (int k = 0; k < 2; k++) {
		if (!want[k]) continue;
		void *p = nullptr;
		if (hipMalloc(&p, want[k]) != hipSuccess) { (void)hipGetLastError(); continue; }      // (no reservation: gsa_create allocates as ever)
		std::lock_guard<std::mutex> g(g_res_mu);
		g_res[device & 63][k].p = p; g_res[device & 63][k].bytes = want[k];
	}
	return GSA_OK;
}
void gsa_release_reserved(int device)
{
	void *f[2] = { nullptr, nullptr };
	{ std::lock_guard<std::mutex> g(g_res_mu); for (int k = 0; k < 2; k++) { f[k] = g_res[device & 63][k].p; g_res[device & 63][k].p = nullptr; g_res[device & 63][k].bytes = 0; } }
	if (f[0] || f[1]) { (void)hipSetDevice(device); for (int k = 0; k < 2; k++) if (f[k]) hipFree(f[k]); }
}

// Host-thread placement.  A contig of a few Mb is some sixty short GPU operations with five host look-ins: a host thread on
// the socket the GPU does not hang off pays the inter-socket hop on every doorbell, pinned-memory poll and count read-back
// (measured on a two-socket MI355X host with the whole process placed by taskset, 5 Mb contigs, three contexts: 0.86 ms per
// contig from the far socket, 0.65 - 0.75 from the near one.  NOT applied by default anywhere: 250 Mb contigs ran 5 % slower with
// the driving threads bound -- 14.4 against 13.7 ms per step on the same box -- so placement is the integrator's decision).  The CPUs local to the device come from sysfs (local_cpulist of its PCI function).
static bool device_local_cpus(int device, cpu_set_t *set)
{
	char bus[64] = { 0 };
	if (hipDeviceGetPCIBusId(bus, (int)sizeof(bus) - 1, device) != hipSuccess) { (void)hipGetLastError(); return false; }
	for (char *p = bus; *p; p++) if (*p >= 'A' && *p <= 'Z') *p = (char)(*p - 'A' + 'a');
	char path[160]; snprintf(path, sizeof(path), "/sys/bus/pci/devices/%s/local_cpulist", bus);
	FILE *f = fopen(path, "r"); if (!f) return false;
	char line[4096]; const bool got = fgets(line, sizeof(line), f) != nullptr; fclose(f);
	if (!got) return false;
	CPU_ZERO(set); int n = 0;
	for (char *p = line; *p;) {
		while (*p == ',' || *p == ' ' || *p == '\n') p++;
		if (!*p) break;
		char *e; long a = strtol(p, &e, 10), b = a; if (e == p) break;
		if (*e == '-') { p = e + 1; b = strtol(p, &e, 10); if (e == p) break; }
		for (long k = a; k <= b && k < CPU_SETSIZE; k++) { CPU_SET((int)k, set); n++; }
		p = e;
	}
	return n > 0;
}
int gsa_bind_host_thread(int device)
{
	cpu_set_t set;
	if (!device_local_cpus(device, &set)) return GSA_OK;      // (no topology information: leave the thread where it is)
	(void)pthread_setaffinity_np(pthread_self(), sizeof(set), &set);
	return GSA_OK;
}

// Pinned host memory for query contigs: a FASTA loader that reads into such a buffer makes the upload of
// gsa_align_contig one asynchronous DMA transfer (pageable memory is staged through the runtime's bounce buffers).
void *gsa_host_alloc(size_t bytes)
{
	void *p = nullptr;
	if (hipHostMalloc(&p, bytes ? bytes : 1) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
	return p;
}
void gsa_host_free(void *p) { if (p) (void)hipHostFree(p); }
int gsa_host_register(void *p, size_t bytes)
{
	if (!p || !bytes) return GSA_ERR_ARG;
	if (hipHostRegister(p, bytes, hipHostRegisterDefault) != hipSuccess) { (void)hipGetLastError(); return GSA_ERR_HIP; }
	return GSA_OK;
}
int gsa_host_unregister(void *p)
{
	if (!p) return GSA_ERR_ARG;
	if (hipHostUnregister(p) != hipSuccess) { (void)hipGetLastError(); return GSA_ERR_HIP; }
	return GSA_OK;
}

// device memory for contigs that stay resident (gsa_set_query_device, GSA_MANY_DEVICE)
void *gsa_device_alloc(int device, size_t bytes)
{
	void *p = nullptr;
	if (hipSetDevice(device) != hipSuccess || hipMalloc(&p, (bytes ? bytes : 1) + 64) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
	return p;
}
void gsa_device_free(int device, void *p) { if (p && hipSetDevice(device) == hipSuccess) (void)hipFree(p); }
int gsa_device_upload(int device, void *dst, const void *src, size_t bytes)
{
	if (!dst || (!src && bytes)) return GSA_ERR_ARG;
	if (hipSetDevice(device) != hipSuccess || hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice) != hipSuccess) { (void)hipGetLastError(); return GSA_ERR_HIP; }
	return GSA_OK;
}

// Test hooks "dbg_*": the launch counters that are never reset (DESIGN, "Counters that are never reset"), put where they come round, so that tests/test_gpu_wrap_states.py
// runs the host lines that handle a wrap.  An epoch only moves forward and stays inside its width: the hook itself can make no stale word valid again.  A ticket takes
// any value, on the host and on the device together.  Nothing of the context is in flight while either changes.
static int dbg_set_launch_counter(gsa_ctx *c, const std::string &k, int64_t value)
{
	GSA_CHECK(c, hipSetDevice(c->device));
	ctx_quiesce(c);
	if ((k == "dbg_walk_epoch" || k == "dbg_walk_ticket") && !c->w_j0.p) return gsa_fail(c, GSA_ERR_STATE, k + ": no window chain has been walked in slices yet (the first one starts both counters at zero)");
	u32 *epoch = k == "dbg_dp_epoch" ? &c->dp_epoch : k == "dbg_band_epoch" ? &c->band_epoch : k == "dbg_lb_epoch" ? &c->lb_epoch : k == "dbg_walk_epoch" ? &c->walk_epoch : nullptr;
	if (epoch) {
		const int64_t top = k == "dbg_dp_epoch" ? 0xffffll : k == "dbg_lb_epoch" ? 0x3fffffffll : 0xffffffffll;
		if (value < (int64_t)*epoch || value > top) return gsa_fail(c, GSA_ERR_ARG, k + ": " + std::to_string((long long)*epoch) + " (the counter's value: it only moves forward) .. " + std::to_string((long long)top));
		*epoch = (u32)value;
		return GSA_OK;
	}
	if (value < 0 || value > 0xffffffffll) return gsa_fail(c, GSA_ERR_ARG, k + ": 0 .. 2^32 - 1");
	const u32 v = (u32)value;
	if (k == "dbg_lb_ticket") { GSA_CHECK(c, hipMemcpy(c->d_mail.as<u32>() + M_TICKET, &v, 4, hipMemcpyHostToDevice)); c->lb_base = v; }
	else { GSA_CHECK(c, hipMemcpy(c->w_j0.p, &v, 4, hipMemcpyHostToDevice)); c->walk_ticket = v; }
	return GSA_OK;
}

int gsa_set_option(gsa_ctx *c, const char *name, int64_t value)
{
	if (!c || !name) return GSA_ERR_ARG;
	const std::string k(name);
	auto in = [&](int64_t lo, int64_t hi) { return value >= lo && value <= hi; };
	const int64_t BIG = (int64_t)1 << 40;
	if (k == "split_min") { if (!in(0, BIG)) return gsa_fail(c, GSA_ERR_ARG, "split_min: 0 .. 2^40 bases"); c->opt.split_min = value; }
	else if (k == "bundle_contig") { if (!in(0, BIG)) return gsa_fail(c, GSA_ERR_ARG, "bundle_contig: 0 (no bundles) .. 2^40 bases"); c->opt.bundle_contig = value; }
	else if (k == "bundle_cap") { if (!in(1, BIG)) return gsa_fail(c, GSA_ERR_ARG, "bundle_cap: 1 .. 2^40 bases"); c->opt.bundle_cap = value; }
	else if (k == "seed_budget") { if (!in(1, 0xffffffffll)) return gsa_fail(c, GSA_ERR_ARG, "seed_budget: 1 .. 2^32 - 1 wave-iterations"); c->seed_budget = (u32)value; }
	else if (k == "dp_lane") { if (!in(0, 1 << 20)) return gsa_fail(c, GSA_ERR_ARG, "dp_lane: 0 (no lane class: one per wavefront) .. 2^20 cells"); c->opt.dp_lane = (int)value; }
	else if (k == "seed_mode") { if (value < 0 || value > 2) return gsa_fail(c, GSA_ERR_ARG, "seed_mode: 0 sweep, 1 speculative, 2 search"); c->opt.seed_mode = (int)value; }
	else if (k == "seed_lhop") { if (value != 0 && (!in(16, 1 << 16) || (value & (value - 1)))) return gsa_fail(c, GSA_ERR_ARG, "seed_lhop: 0 or a power of two >= 16"); c->opt.seed_lhop = (int)value; }    // (test hook: a smaller long-hop table)
	else if (k == "pd_bitmap") c->opt.pd_bitmap = value != 0;
	else if (k == "dp_side") c->opt.dp_side = value != 0;
	else if (k == "dp_pair") { if (!in(0, 3)) return gsa_fail(c, GSA_ERR_ARG, "dp_pair: 0 never, 1 where it costs fewer wave-steps in a long class, 2 always, 3 where it costs fewer wave-steps"); c->opt.dp_pair = (int)value; }
	else if (k == "dp_band") { if (!in(0, 2)) return gsa_fail(c, GSA_ERR_ARG, "dp_band: 0 never, 1 where the band costs at most 3/4 of the striped wave-steps, 2 every job the layout admits"); c->opt.dp_band = (int)value; }
	else if (k == "dp_band_margin") { if (!in(1, 63)) return gsa_fail(c, GSA_ERR_ARG, "dp_band_margin: 1 .. 63 diagonals"); c->opt.dp_band_margin = (int)value; }
	else if (k == "pd_two_level_min") { if (!in(0, BIG)) return gsa_fail(c, GSA_ERR_ARG, "pd_two_level_min: >= 0 blocks"); c->opt.pd_two_level_min = value; }
	else if (k == "pd_bytes") { if (!in(0, 2)) return gsa_fail(c, GSA_ERR_ARG, "pd_bytes: 0 never, 1 by the hit count, 2 always"); c->opt.pd_bytes = (int)value; }
	else if (k == "pres_from_kmer") c->opt.pres_from_kmer = value != 0;      // (takes effect at the next gsa_set_params that rebuilds the table)
	else if (k == "walk_chain_min") { if (!in(0, BIG)) return gsa_fail(c, GSA_ERR_ARG, "walk_chain_min: >= 0 seeds"); c->opt.walk_chain_min = value; }
	else if (k == "sweep_shape") { if (value < -1 || value > 1) return gsa_fail(c, GSA_ERR_ARG, "sweep_shape: -1, 0 or 1"); c->opt.sweep_shape = (int)value; }
	else if (k == "dp_safe") c->dp_safe = value != 0;                    // (test hook)
	else if (k == "dp_fake_timeout") { if (!in(0, 1 << 20)) return gsa_fail(c, GSA_ERR_ARG, "dp_fake_timeout: >= 0"); c->dp_fake_timeout = (int)value; }    // (test hook)
	else if (k == "dbg_dp_epoch" || k == "dbg_band_epoch" || k == "dbg_lb_epoch" || k == "dbg_walk_epoch" || k == "dbg_lb_ticket" || k == "dbg_walk_ticket") return dbg_set_launch_counter(c, k, value);    // (test hooks)
	else return gsa_fail(c, GSA_ERR_ARG, "gsa_set_option: unknown option " + k);
	return GSA_OK;
}

// The device buffers of a context, largest first, to stderr: name, bytes held, bytes last asked for (diagnosis: what a context's share of HBM is made of).
int gsa_debug_buffers(gsa_ctx *c, int top)
{
	if (!c) return GSA_ERR_ARG;
	struct E { const char *name; size_t cap, len; };
	std::vector<E> v;
#define X(n) if (c->n.p) v.push_back({ #n, c->n.cap, c->n.len });
	GSA_DEVBUFS(X)
#undef X
	std::sort(v.begin(), v.end(), [](const E &a, const E &b) { return a.cap > b.cap; });
	size_t tot = 0; for (const E &e : v) tot += e.cap;
	fprintf(stderr, "[gsa_debug_buffers] %zu device buffers, %.2f GB held\n", v.size(), (double)tot / 1e9);
	for (size_t k = 0; k < v.size() && (int)k < top; k++) fprintf(stderr, "  %-16s %10.1f MB held  %10.1f MB asked\n", v[k].name, (double)v[k].cap / 1e6, (double)v[k].len / 1e6);
	return GSA_OK;
}

// ---- the index builder (k_index.hip) ----
int gsa_index_sizes(int64_t G, uint64_t *bwt_words, uint64_t *n_sa)
{
	if (G <= 0 || !bwt_words || !n_sa) return gsa_fail(nullptr, GSA_ERR_ARG, "gsa_index_sizes: bad argument");
	const uint64_t S = 2 * (uint64_t)G;
	*bwt_words = (S + 15) / 16 + ((S + 127) / 128 + 1) * 8;
	*n_sa = (S + 32) / 32;
	return GSA_OK;
}
static thread_local IxStats g_ix;      // the calling thread's last build
// A context with no index: the device, one stream, the mailbox the fused passes draw their tickets from; the sort's scratch (tmp) and the look-back status words
// grow on first use.  No uploader thread, no events, no auxiliary streams.  gsa_destroy frees it like any other context.
static int ix_bare_ctx(const char *who, int device, gsa_ctx **out)
{
	gsa_ctx *c = new gsa_ctx();
	c->device = device;
	hipError_t e = hipSetDevice(device);
	if (e == hipSuccess) e = hipStreamCreate(&c->stream);
	if (e == hipSuccess) e = hipMalloc(&c->d_mail.p, MAIL_N * sizeof(i32));
	if (e == hipSuccess) { c->d_mail.cap = MAIL_N * sizeof(i32); e = hipMemset(c->d_mail.p, 0, MAIL_N * sizeof(i32)); }
	if (e != hipSuccess) { (void)hipGetLastError(); return ctx_abandon(c, GSA_ERR_HIP, std::string(who) + ": device set-up: " + hipGetErrorString(e)); }
	*out = c;
	return GSA_OK;
}
// both entry points behind their argument checks: a bare context, the build, its figures, the context gone
static int ix_build(const char *who, int device, const uint8_t *pac, int64_t G, const IxOpts &o, uint64_t *primary, uint64_t L2[5], uint32_t *bwt, uint64_t *sa)
{
	if (int rc = create_device_ok(who, device)) return rc;
	gsa_ctx *c = nullptr;
	if (int rc = ix_bare_ctx(who, device, &c)) return rc;
	IxStats s;
	if (int rc = build_index_device(c, pac, G, o, who, primary, L2, bwt, sa, &s)) { g_create_error = c->err; return ctx_abandon(c, rc); }
	g_ix = s;
	gsa_destroy(c);
	return GSA_OK;
}
int gsa_build_index(int device, const uint8_t *pac, int64_t G, uint64_t *primary, uint64_t L2[5], uint32_t *bwt, uint64_t *sa)
{
	if (!pac || !primary || !L2 || !bwt || !sa || G <= 0) return gsa_fail(nullptr, GSA_ERR_ARG, "gsa_build_index: bad argument");
	// 32-bit suffix indices, ranks and scatter positions: the text with its '$' has at most 2^31 - 2 suffixes (the bound of the host builder's 32-bit instance)
	if (2 * G + 1 > (1ll << 31) - 2) return gsa_fail(nullptr, GSA_ERR_LIMIT, "gsa_build_index: the reference is longer than 1 073 741 822 bases (the device builder sorts 32-bit suffix indices)");
	return ix_build("gsa_build_index", device, pac, G, IxOpts{ false, 0, 0, 0 }, primary, L2, bwt, sa);
}
int gsa_build_index_opts(int device, const uint8_t *pac, int64_t G, uint32_t flags, int64_t batch_cap, int64_t occ_segment, uint64_t *primary, uint64_t L2[5], uint32_t *bwt, uint64_t *sa)
{
	if (!pac || !primary || !L2 || !bwt || !sa || G <= 0) return gsa_fail(nullptr, GSA_ERR_ARG, "gsa_build_index_opts: bad argument");
	if (flags & ~(uint32_t)GSA_BUILD_WIDE) return gsa_fail(nullptr, GSA_ERR_ARG, "gsa_build_index_opts: unknown flag");
	if (batch_cap < 0 || occ_segment < 0) return gsa_fail(nullptr, GSA_ERR_ARG, "gsa_build_index_opts: batch_cap and occ_segment are 0 (the default) or positive");
	if (G > IX_WIDE_MAX_G) return gsa_fail(nullptr, GSA_ERR_LIMIT, "gsa_build_index_opts: the reference is longer than 4 294 967 295 bases (the wide device builder's sort key holds a 33-bit rank)");
	const bool wide = (flags & GSA_BUILD_WIDE) != 0 || 2 * G + 1 > (1ll << 31) - 2;
	if (!wide) return gsa_build_index(device, pac, G, primary, L2, bwt, sa);
	return ix_build("gsa_build_index_opts", device, pac, G, IxOpts{ true, batch_cap, occ_segment, g_ix_active_cap.load() }, primary, L2, bwt, sa);
}
int gsa_get_index_build_stats2(int64_t *batches, uint64_t *peak_bytes, int64_t *active_suffixes)
{
	if (!batches || !peak_bytes || !active_suffixes) return GSA_ERR_ARG;
	*batches = g_ix.batches; *peak_bytes = g_ix.peak; *active_suffixes = g_ix.active;
	return GSA_OK;
}
int gsa_set_index_build_caps(int64_t batch_cap, int64_t occ_segment, int64_t active_cap)
{
	if (batch_cap < 0 || occ_segment < 0 || active_cap < 0) return gsa_fail(nullptr, GSA_ERR_ARG, "gsa_set_index_build_caps: 0 (the default) or positive");
	g_ix_batch_cap.store(batch_cap); g_ix_occ_segment.store(occ_segment); g_ix_active_cap.store(active_cap);
	return GSA_OK;
}
int gsa_get_index_build_stats(double *ms, int32_t *rounds)
{
	if (!ms || !rounds) return GSA_ERR_ARG;
	*ms = g_ix.ms; *rounds = g_ix.rounds;
	return GSA_OK;
}
} // extern "C"
