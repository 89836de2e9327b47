// gsalign_amd/csrc/gsa_ctx.h -- the context behind the opaque gsa_ctx handle.
#ifndef GSA_CTX_H
#define GSA_CTX_H
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <thread>
#include "gsa_internal.h"

// A leaf = a maximal run of seeds of one S2 block that neither S4 (large gaps)
// nor S5 (reference chromosome ends) cuts.  Host-side block bookkeeping works on
// ranges of leaves.
struct Leaf {
	i32 beg, end;        // seed range in the refined seed arrays
	i32 sumlen;          // sum of (trimmed) seed lengths
	i32 q_first, q_last_end;
	i64 r_first, r_last_end;
	i32 blk;             // S2 block this leaf belongs to
	i32 cut4, cut5;      // how this leaf starts: S4 cut / S5 cut (0/0 = block start)
	i32 blk_score;       // AddAlnBlock score of that S2 block
};

// Device "mailbox" (i32[MAIL_N]) of the counts the stages produce; the host reads the whole
// box in ONE pinned copy where it needs them instead of one read-back per count.
enum { M_NB = 0, M_NC = 1, M_NBLK = 2, M_NG = 3, M_NR = 4, M_NJ = 5, M_NL = 6, M_LBERR = 7, M_ANY = 8, M_NLANE = 40, M_TICKET = 48, M_NBRAW = 49, M_NR2 = 50, M_NF = 51, M_NJOB = 52, M_OPSTOT = 53, M_NALN = 54, M_DPERR = 64, M_NLARGE = 65, M_DPERR2 = 66, M_CELLS = 68 /* two u64: sum m*n, sum m+n */ /* 64..71: cleared together, one aligned 32-byte fill */, M_DPERR3 = 41, M_LBDONE = 42, M_LFSTEPS = 44 /* u64, accounting build */, M_NEARLY = 62, M_EOPS = 63, M_NTOUCH = 46 /* touched PosDiff-bitmap blocks (OpPdTouched) */, M_MAXBLK = 56 /* u64 {score, number} of the best-scoring stage-2 block */, MAIL_N = 72 };
#define LEAF_CHUNK 1024      // leaves copied together with the mailbox (more -> a second copy)

struct HostBlock {       // one entry of the reference's AlnBlockVec, as leaf range
	i32 leaf_beg, leaf_end;
	i32 score;
	i32 bdup;
	// filled at stage 8
	i32 aln_len, bdir, gpos, chr;
};

// A query slot: the device copy of a contig, or of a bundle's concatenation with its tables.  A context has two: while the contig
// of one slot goes through the stages, the next one is uploaded into the other by the Uploader's thread and copy stream (gsa_prefetch_contig /
// gsa_prefetch_bundle; gsa_align_many does it by itself), so the H2D copy of a contig -- 4.8 ms for 250 Mb at 52 GB/s, the reference
// reads QueryChrVec[i].seq from host memory every iteration (GSAlign.cpp:483-490) -- hides behind its predecessor's stages.
struct QuerySlot {
	DevBuf d_query;                                // contig / concatenation
	DevBuf d_bndtab, p_bndtab;                     // bundle tables: off[n + 1] | chunk_contig[chunks] | (device-resident contigs: source pointers) -- device / pinned staging
	std::vector<i32> b_off, b_qlen;                // start of contig k in the concatenation [n + 1], its length
	std::vector<const char *> src;                 // the host buffers this slot was filled from (the identity of a prefetch)
	i32 n = 0;                                     // 0: one contig, > 0: a bundle of n
	i32 lmax = 0; i64 tot = 0; size_t o_cc = 0, o_src = 0;
	bool pending = false;                          // uploaded (or on its way) and not yet adopted by gsa_set_query / set_query_bundle
	std::atomic<int> busy{0};                      // uploads of this slot the Uploader has not finished yet
	std::atomic<int> up_err{0};                    // first hipError_t of an upload into this slot (the Uploader thread sets it, slot_finish turns it into GSA_ERR_HIP)
};
static inline void slot_wait(QuerySlot &s) { while (s.busy.load(std::memory_order_acquire) > 0) std::this_thread::yield(); }      // (the slot functions of gsa_query.hip, gsa_destroy)

// Uploads of query sequences, ONE AT A TIME per device index, in the order they were asked for (a thread + a copy stream; the contexts
// that share an index -- gsa_clone -- share it).  Why not a copy stream per context: copies that run side by side share the link, so
// every one of them takes as long as all of them together; four contexts that each prefetch their next contig then all get it late, at
// the same moment, and stay in lockstep (measured: the host waited 5 ms per contig for an upload issued a whole contig earlier, and the
// upload-inclusive rate was 27.5 Gbp/s against 31.5 with resident contigs).  First come first served, a 250 MB contig lands 4.4 ms after
// its turn and the contexts stagger.  Nothing but DMA copies runs on the stream and only host threads wait for them: a GPU-side wait
// (an event behind the copy, a kernel queued behind it) is a barrier packet that blocks a shared hardware queue for milliseconds.
struct Uploader {
	struct Piece { void *dst; const void *src; size_t n; };
	struct Job { std::vector<Piece> pieces; std::atomic<int> *busy; std::atomic<int> *err; std::chrono::steady_clock::time_point t_push; };
	double copy_ms = 0, wait_ms = 0, bytes = 0; long long jobs = 0;      // (statistics, uploader thread only)
	int device = 0; hipStream_t st = nullptr;
	std::thread th; std::mutex mu; std::condition_variable cv; std::deque<Job> q; bool stop = false;
	size_t n_demand = 0;                           // the first n_demand jobs of q are uploads a context is waiting for (slot_demand), in the order they asked
	void run();
	void push(Job &&j) { j.busy->fetch_add(1); j.t_push = std::chrono::steady_clock::now(); { std::lock_guard<std::mutex> g(mu); q.push_back(std::move(j)); } cv.notify_one(); }
};

// What gsa_set_option sets (include/gsa_hip.h); a clone starts with its parent's values.  The library reads NO environment variable
// (experiment switches exist only in builds with -DGSA_EXPERIMENTS).
struct Options {
	int64_t split_min = 20000000;      // gsa_align_many: a contig of at least this many bases may be seeded by chunk range on several contexts
	int64_t bundle_contig = 16000000;  // ... contigs up to this length travel in bundles (0: never)
	int64_t bundle_cap = 64000000;     // ... of about this many bases at most
	int dp_lane = 512;                 // alignments of at most this many cells go one per lane (k_dp_lane); 0: no lane class, every job below the striped kernel runs one per wavefront (k_dp_small)
	int seed_lhop = 0;                 // (test hook) entries of the seed kernel's long-hop table a chunk may use: a power of two below LHOP_N; 0 = all of them
	int seed_mode = 1;                 // 0 sweep: every chunk through k_dense_sweep; 1: the speculative kernel + dense kernels for what it gives up on; 2: round 2's k_dense_search in place of the sweep
	int pd_bitmap = 1;                 // 0: groups by the PosDiff sort although MaxIndelSize <= 31 would allow the bitmap scan
	int sweep_shape = -1;              // k_dense_sweep's launch shape: -1 by the number of dense chunks, 0 = four chunks per two-wave workgroup / 160-start segments, 1 = one chunk per four-wave workgroup / 40-start segments
	int dp_side = 0;                   // 1: the striped DP's lower size class on a stream of its own, beside the upper class (0: behind it)
	int dp_pair = 1;                   // the striped DP runs two jobs side by side in a wave's 16-bit halves: 0 never (every job in the lagged form), 1 where that costs fewer wave-steps, in size classes of at least DP_PAIR_MIN_JOBS jobs, 2 every two neighbours of a size class, 3 as 1 in a class of any length (2, 3: tests)
	int dp_band = 1;                   // near-diagonal striped jobs run in k_dp_band first and keep its result where the certificate holds: 0 never, 1 where the band costs at most 3/4 of the striped form's wave-steps, 2 every job the layout admits (tests)
	int dp_band_margin = 32;           // B: the band certified is the diagonals [min(0, n - m) - B, max(0, n - m) + B]
	int64_t walk_chain_min = 100000;   // contigs with more seeds than this walk their window chain in slices (k_walk_chain) instead of one workgroup's LDS (k_walk_windows); tests: 0
	int64_t pd_two_level_min = 2000000;   // PosDiff bitmaps of more blocks than this (a reference above ~1 Gbp) are scanned in two passes: list the touched blocks, count those (tests: 0)
	int pd_bytes = 1;                  // the PosDiff bitmap of a contig (bundle) whose hits scatter (-sen: thousands of chance hits per chunk) is filled through a byte per value, plain stores, and packed
	                                   // afterwards -- no device-scope atomics (k_pd_pack, k_seed_select.hip); 1 = when the hit count says so, 0 = never, 2 = always (tests)
	int pres_from_kmer = 1;            // the presence table is derived from the k-mer jump table when both hold k-mers of one length (0: always from a scan of the text; a test compares the two)
	int kmer_k = 0;                    // gsa_create_opts (GSA_CREATE_KMER_K): length of the jump table's k-mers (0: by text length and free memory)
};

// The dense per-reference-base accumulator of gsa_project (k_proj.hip): one word per forward reference position on one device, shared by the contexts
// that opened it (gsa_proj_open) and freed by the last one that lets go of it.  dirty: a pass that failed left words behind that nobody vouches for.
struct ProjAcc { u32 *words = nullptr; i64 G = 0; int device = 0; std::atomic<int> refs{1}; std::atomic<int> dirty{0}; };

// the passes over a stage-8 result, as gsa_ctx::pass_stat counts them
enum Pass { PASS_VAR, PASS_CIG, PASS_CS, PASS_LIFT, PASS_TRACK, PASS_SEG, PASS_PROJ, PASS_REG, PASS_QTRACK, PASS_N };
struct PassStat { double ms_sum = 0; long long calls = 0; };

struct gsa_ctx {
	int device = 0;
	Options opt;
	Uploader *up = nullptr; bool own_up = false;
	hipStream_t stream = nullptr;
	hipStream_t stream_seed = nullptr;      // GSA_CREATE_PRIO: the seed-search kernels on a stream of their own, so that they do not inherit the main stream's priority (ctx_private_init); else null
	hipEvent_t ev_seed_fork = nullptr;
	u64 seed_ticket = 0;                    // value of the seed kernel's ticket counter (d_cnt[16]) before the next launch
	int n_cus = 0;
	bool seed_lds_checked = false;       // stage1_seed compared the LDS its launch asks for with the device's per-block limit
	hipStream_t stream_aux[4] = {nullptr, nullptr, nullptr, nullptr};   // [3]: a striped size class's unpaired jobs beside its pairs (launch_stripes; default path on contigs with a class of DP_PAIR_MIN_JOBS jobs), and the lower size class beside the upper one (option dp_side); [0] early striped DP, [1] tiny DP + strings + sums, [2] records to the host (five streams with the main one: with the runtime's default of four hardware queues two of them share one; bench.py asks for 16)
	std::string err;
	Params prm;
	DevIndex di = {};
	gsa_ctx *index_owner = nullptr;                // gsa_clone: the context whose device index this one borrows (nullptr = own)
	gsa_ctx *lender = nullptr;                     // gsa_clone: the context `di` was copied from -- its presence bitmap / short k-mer table are read through that copy
	std::atomic<int> n_borrowers{0};               // live clones made FROM this context (gsa_set_params must not rebuild the tables they read)
	int prio_mode = 0;                             // GSA_CREATE_PRIO: stream priorities (0: none; see ctx_private_init)
	bool force_wide = false;                       // GSA_CREATE_WIDE: 64-bit dense SA + 32-byte k-mer entries whatever the text length (the >= 2^32-row layout)
	bool profiling = false;
	bool prof_seed = false;                        // time the seed kernel only (two events instead of ten per contig)
	bool count_blocks = false;                     // run the accounting build of the seed kernel (exact algorithmic Occ-block count)
	u64 dbg[8] = {0, 0, 0, 0, 0, 0, 0, 0};
	hipEvent_t ev[28] = {};
	float kernel_ms[8] = {};
	double wall_ms[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; int64_t wall_n = 0;      // host wall clock spent in [0] the query set-up (upload / wait for the prefetch) and [s] stage s of gsa_run_to, summed over contigs since gsa_set_profiling (gsa_get_wall_sums)
	double acc_seed_ms = 0.0;                      // seed-search kernel time summed over the contigs since gsa_set_profiling (flag bit 2), see gsa_get_timings
	u64 counters[8] = {};
	u64 dp_stats[4] = {};                          // launch_stripes since the context was made: striped jobs, of them side by side, lagged launches, side-by-side launches (gsa_get_dp_stats)

	// index (device)
	DevBuf d_bwt, d_bwt_ref, d_occ_base, d_sa, d_ref, d_chr_end, d_chr_of_end;
	std::vector<i64> h_chr_end, h_chr_fwd; std::vector<i32> h_chr_of_end, h_chr_len;
	i64 G = 0;

	// query
	QuerySlot qs[2]; int q_cur = -1;               // q_cur: slot of the current contig; -1: the caller's device buffer / none; -2: overwritten by a prefetch (no gsa_rewind)
	i32 qlen = 0; int stage = 0;
	const uint8_t *q_dev = nullptr;                // the contig on the device: d_query (uploaded by gsa_set_query) or the caller's buffer (gsa_set_query_device)
	bool split = false; i64 rng_beg = 0, rng_end = 0;     // gsa_seed_chunks: stage 1 on a chunk range only, the hits of other ranges are imported
	int qbits = 1, pdbits = 1;
	i64 pd_span = 0;                               // number of PosDiff key values: 2G + qlen + 2, a bundle: contigs x stride

	// ---- a bundle of contigs in one pass (Bundle, gsa_internal.h; gsa_align_bundle in gsa_api.hip, set_query_bundle in gsa_query.hip) ----
	Bundle bnd = { 0, 0, 0, nullptr, nullptr }; bool bundle_call = false;
	std::vector<i32> b_off, b_qlen;               // start of contig k in the concatenation [n + 1], its length (copied from the slot that holds the bundle)
	std::vector<std::vector<HostBlock> > b_lists;  // the AlnBlockVec of every contig while the list logic runs (stages 3-6)
	std::vector<i32> b_blk0;                       // first block of contig k in the joined final list [n + 1]
	DevBuf d_bblk, p_bblk, p_ba0;                          // contig of every final block | first block per contig (device); string-pool offset of every contig (pinned, written by k_bundle_rebase)
	std::vector<i32> b_nblk; std::vector<i64> b_frag0;      // blocks that survive the identity filter, and the first record, per contig

	// scratch for rocPRIM
	DevBuf tmp;
	DevBuf leaf[9];                                // device staging of the leaf operators' batches (kept: a batch call allocates nothing once warm)
	// device counters block (u64[16]) + pinned host mirror
	DevBuf d_cnt; u64 *h_cnt = nullptr;
	DevBuf d_mail; i32 *h_mail = nullptr;          // count mailbox + pinned mirror
	DevBuf d_lb_status[2]; u32 lb_epoch = 0, lb_base = 0;   // look-back scan state (gsa_scan.h); the ticket counter sits in the mailbox
	DevBuf p_leaf;                                 // pinned landing zone for the leaf table
	int ev_pending = 0;                            // bit0: stage-1 events, bit1: stage-2 events not yet read
	bool s2_host = false;                          // n_b/n_c/n_blocks2/h_blk_* fetched for the stage-2 view

	// ---- stage 1 ----
	DevBuf d_ref2;                                 // 2-bit packed reference text
	DevBuf d_kmer;                                 // top-of-tree jump table
	DevBuf d_kmer_lo;                              // its short companion (MinSeedLength bases), see DevIndex::kmer_lo
	DevBuf d_pres;                                 // MinSeedLength-mer presence bitmap
	DevBuf d_sa_dense;                             // one SA entry per BWT row (built at gsa_create)
	DevBuf d_cand_s, d_cand_len, d_cand_x0, d_cand_freq, d_onpath, d_cand_cnt;
	size_t cand_cap_per_chunk = 1536;
	DevBuf d_heavy, dn_lf, dn_x0;               // chunks the speculative seed kernel gave up on; next(s) / accepted match per start of the dense chunks
	bool seed_sweep_next = false, seed_sweep_probe = false; int seed_sweep_run = 0, seed_sweep_period = 8;   // the previous contig handed most chunks to the sweep: the next one starts there (k_seed.hip, stage1_seed)
	u32 seed_budget = 256;                         // wave-iterations a chunk may take in the speculative kernel before it goes to the dense path (GSA_SEED_BUDGET)
	DevBuf d_chunk_hits, d_chunk_base;             // located hits per chunk and their exclusive prefix   // memoised matches of the search kernel + on-path bits
	DevBuf d_key_a, d_key_b, d_val_a, d_val_b;     // sort ping-pong
	i64 n_seeds = 0; bool hits_sorted = false;     // the hits in d_key_a / d_val_a are in (qPos, rank) order (k_seed_select over the whole contig; not after an import)
	DevBuf s_q, s_len, s_r, s_gid;                 // seeds in (PosDiff,qPos) order + group id
	DevBuf d_flag, d_scan;                         // generic i32 flag / scan arrays (n+1)
	i32 n_groups = 0;
	bool pd_path = false, seed_view_ready = false, pdbm_dirty = true; i64 pd_words = 0;      // groups from the PosDiff bitmap (no PosDiff sort on the hot path)
	DevBuf w_j0; u32 walk_ticket = 0, walk_epoch = 0;   // window chain of large contigs (k_walk_chain): ticket counter + one entry word per slice, never reset -- the host passes the counter's value and the launch epoch
	u32 walk_last_epoch = 0;                       // the epoch of the last k_walk_chain launch (0: none yet) -- gsa_get_launch_counters counts the entry words that carry it
	DevBuf d_zero;                                 // 256 zero bytes: Bundle::off / chunk_contig of a context without a bundle
	DevBuf d_pdby; bool pd_bytes = false;          // a byte per PosDiff value (all zero between contigs), see Options::pd_bytes
	DevBuf d_pdcb;                                 // coarse bitmap: one bit per block of 32 words of d_pdbm (the blocks that hold a hit)
	DevBuf d_pdbm, d_gpre, d_key_c, d_val_c;      // bitmap of occupied PosDiff values, group starts below each word, (group, qPos, rank) keys
	DevBuf g_beg;                                  // group start indices (n_groups+1)

	// ---- stage 2 ---- (arrays over seeds of active groups, (group,qPos,rPos) order)
	i64 n_a = 0;
	DevBuf a_q, a_len, a_r, a_gb, a_ge;            // + group begin/end index per seed
	DevBuf a_uniq, a_cu, a_alive, a_ws, a_wid;
	DevBuf a_next, a_brk, a_aurank, a_aulist, a_runinfo;
	DevBuf w_best, w_sum, w_n;
	DevBuf d_btab;                                 // (window, bucket) -> count hash table of the outlier filter
	DevBuf d_flag2, d_scan2, d_i64a;
	i64 n_b = 0, n_c = 0;
	DevBuf b_q, b_len, b_r, b_gb, b_ge;            // after compaction #1
	DevBuf c_q, c_len, c_r, c_gb, c_ge;            // after compaction #2
	DevBuf c_bid;                                  // S2 block id per seed (-1 = none)
	i32 n_blocks2 = 0;
	DevBuf blk_beg, blk_end, blk_score;            // S2 blocks kept by AddAlnBlock
	std::vector<i32> h_blk_beg, h_blk_end, h_blk_score;

	// ---- stages 3-5 ---- refined seed arrays (after RemoveOverlaps)
	i64 n_r = 0;
	DevBuf r_q, r_len, r_r, r_bid, r_tmp_q, r_tmp_len, r_tmp_r, r_tmp_bid;
	DevBuf r_cut4, r_cut5, r_simjob, r_simres;
	DevBuf d_leaf; std::vector<Leaf> h_leaf;
	std::vector<HostBlock> blocks;                 // current AlnBlockVec
	std::vector<i32> h_r_q, h_r_len; std::vector<i64> h_r_r;    // host copies of refined seeds (for getters / emit)
	bool have_host_seeds = false;

	// ---- stages 7-8 ----
	i64 n_frags = 0, n_aln = 0;                    // (n_frags < 0: still in the mailbox, see frags_count())
	i32 n_large = 0;                               // large DP jobs of the current contig (their records are patched on the host)
	DevBuf p_jpatch; i32 n_jobs = 0;               // pinned: record numbers, then string lengths, of the DP jobs of the job list (the host patches its records)
	DevBuf d_tail, p_tail;                         // final mailbox | patch list | string pool 1 | string pool 2: device / pinned (one copy at the end)
	const i32 *h_tmail = nullptr, *h_tpatch = nullptr; char *h_taln1 = nullptr, *h_taln2 = nullptr;      // the parts of p_tail
	i64 nf_ub = 0, span_ub = 0;                    // host-known upper bounds: records, and bases in gaps (ops / gapped strings)
	DevBuf fb_seedbase, fb_sbeg, fb_fragbase;      // per final block
	DevBuf f_rec;                                  // gsa_frag records (device working set)
	DevBuf f_rec16;                                // the same as 16-byte gsa_rec: what goes to the host
	DevBuf f_type, f_mism, f_alnlen, f_job, f_score;
	DevBuf j_frag, j_opsoff, j_nops, d_ops, j_cells;
	DevBuf d_dp_lane_order;                        // k_dp_lane: its order array (the jobs of the one-per-lane class)
	DevBuf d_dp_arena;                             // k_dp_lane: direction nibbles of the alignments in flight (per-wave regions)
	DevBuf d_dp_bnd, d_dp_ctr, d_dp_jobs, d_dp_large;   // striped DP: boundary granules, tickets, job descriptors, (job,m,n) of the large jobs
	// large DP gaps are known once the leaf table exists: they are launched there (stream_aux[0]) and run under stages 6-7
	DevBuf e_id, e_rec, e_list, e_off1, e_off2, e_opsoff, e_nops, e_ops, e_rev, r_head, f_early, r_orig, r_tmp_orig, p_early;
	bool early_consumed = false;                   // stage 7 enqueued its wait for the early launch (else gsa_run_to waits before it returns)
	bool early_listed = false;                     // stage 2 left the list of large gaps on its way to the host (event ev[16])
	i32 n_early = 0; bool early_in_flight = false; std::vector<i32> h_early;      // (seed, m, n) per early job
	bool dp_dirty = true;                          // ticket counters / error words of the striped DP need clearing (fresh buffer, or a failed launch)
	bool dp_timeout = false, dp_safe = false;      // a striped launch tripped its wait bound; repeat the contig with one job per launch
	int dp_fake_timeout = 0;                       // test hook (GSA_DP_FAKE_TIMEOUT=n at gsa_create): the next n contigs report a hand-off time-out once, so the retry paths run
	u32 dp_epoch = 0;                              // tag of the boundary granules of the current striped launch
	DevBuf d_band_dir, d_band_seq, d_band_cert, d_band_stat;   // band DP (k_dp_band.hip): direction nibbles, the pairs' code strings, {certified tag per job, "has an N" per pair}, the certified-jobs counter
	u32 band_epoch = 0;                            // tag of the certified flags of the current band launch
	u64 band_eligible = 0;                         // jobs given to k_dp_band since the context was made (gsa_get_dp_band_stats)
	DevBuf p_dp, p_sj, p_sj_early;                 // pinned: mailbox + large-job list; stripe job tables (read by the kernels in place)
	DevBuf d_alnoff;
	DevBuf bl_alnlen, bl_score;
	std::vector<gsa_rec> h_frags; std::vector<gsa_block> h_blocks; std::vector<char> h_aln1, h_aln2;
	int frags_stage = 0;                           // stage for which h_frags/h_blocks were built
	// stage-8 results land in pinned host memory (one async D2H each, no pageable staging)
	DevBuf p_frags, p_blk; bool result_pinned = false;
	// ---- variants (k_variants.hip): block table, per-record counts, per-workgroup sums + kind counters, the output; pinned: block table, header {n, kinds}, output ----
	DevBuf d_vblk, d_vcnt, d_vwg, d_var, p_vblk, p_vhdr, p_var;
	bool prof_var = false; hipEvent_t ev_var[2] = {nullptr, nullptr};
	// time and calls per pass (gsa_get_*_timing).  PASS_VAR: device time of the variant passes between its two events, since gsa_set_profiling; every other entry: host
	// wall time inside the export (a cs / segs call's CIGAR pass included), always on -- two clock reads per call -- and never reset
	PassStat pass_stat[PASS_N];
	// ---- per-block CIGARs (k_cigar.hip): block table in / out, per-record run-start and column counts, per-workgroup sums, their prefix sums, the run starts {column << 4 | class}, the ops;
	// pinned: block table in, header {ops, columns, records without a job}, block table out, ops ----
	DevBuf d_cblk, d_cout, d_ccnt, d_cwg, d_cpre, d_crun, d_cops, p_cblk, p_chdr, p_cout, p_cops;
	// ---- per-block cs strings (k_cs.hip): the runs' first positions (written by the CIGAR walk, block_cigars(.., pos)), per-op byte counts, per-workgroup sums, the ops' offsets,
	// block table out, the bytes; pinned: header {bytes, blocks too long, bases out of range}, block table out, the bytes ----
	DevBuf d_crpos, d_cqpos, d_slen, d_swg, d_spre, d_sout, d_cs, p_shdr, p_sout, p_cs;
	// ---- lifted reference positions (k_lift.hip): the positions of gsa_lift_set, the span table sorted by start and per position {chosen table entry, n_cover} (both
	// k_regions.hip's too: a call builds them and has consumed them before it returns), per-workgroup sums + error counters, the hits; pinned: span table, header {hits,
	// records without a job, positions outside their record}, the hits ----
	DevBuf d_lpos, d_lblk, d_lpick, d_lwg, d_lhit, p_lblk, p_lhdr, p_lhit;
	i64 lift_n = 0;                                      // positions held (0: none; a clone starts without)
	// ---- per-window reference track (k_track.hip): the counted blocks' table, the merged intervals, the dense per-window counts {n_eq, n_x, n_del, n_ins} (all zero between
	// calls: EMIT clears what it reads), per-workgroup sums + error counters, the windows; pinned: block table, intervals, header {windows, records without a job, columns
	// outside their record}, the windows ----
	DevBuf d_tblk, d_tiv, d_tbin, d_twg, d_tout, p_tblk, p_tiv, p_thdr, p_tout;
	i32 track_w = 0; i64 track_nwin = 0;                 // window length (0: none; a clone starts without) and the windows of the whole reference at that length
	size_t track_zeroed = 0; bool track_dirty = false;   // entries of d_tbin known to be zero; a call that failed between COUNT and EMIT left counts behind
	// ---- per-block chain segments (k_segs.hip): per-workgroup sums + error counter, segment starts in front of every run, the segments' boundaries {start position,
	// first column, end column, query position}, the blocks' table, the triples; pinned: header {segments, triples that are no chain line}, block table, triples ----
	DevBuf d_sgwg, d_sgpre, d_sgbnd, d_sgout, d_sgseg, p_sghdr, p_sgout, p_sgseg;
	// ---- the query projected onto the reference (k_proj.hip): the accumulator this context paints into (null: none; a clone starts without), the painted blocks' table,
	// per-record prefix of the run records' trimmed columns (entry [W]: their sum), per-workgroup sums + counters, device staging of fetch (characters) and merge (words);
	// pinned: block table, header {run columns, records without a job, columns outside their record or sequence, gap columns}, staging of fetch and merge ----
	ProjAcc *proj = nullptr; u32 proj_flags = 0;
	DevBuf d_pblk, d_ppre, d_pwg, d_pstage, p_pblk, p_phdr, p_pstage;
	// ---- lifted reference intervals (k_regions.hip; table and picks: the lift pass's d_lblk / d_lpick / p_lblk): the regions of gsa_regions_set (n begs, then n ends),
	// the per-record prefix of the four class counts, per-workgroup sums + error counters, the hits; pinned: header {hits, records without a job, spans outside their
	// records}, the hits ----
	DevBuf d_rgpos, d_rgpre, d_rgwg, d_rghit, p_rghdr, p_rghit;
	i64 reg_n = 0;                                       // regions held (0: none; a clone starts without)
	// ---- per-window query track (k_qtrack.hip): the counted blocks' span table, both interval lists (depth >= 1 with its sentinel, then depth >= 2), the dense per-window
	// counts {n_eq, n_x, n_ins, n_del} of ONE contig (all zero between calls: EMIT clears what it reads), per-workgroup sums + error counters, the windows, the gap records
	// that hold a block's cut with their answers; pinned: span table, intervals, header {windows, records without a job, columns outside their record}, the windows, the cuts ----
	DevBuf d_qblk, d_qiv, d_qbin, d_qwg, d_qout, d_qcut, p_qblk, p_qiv, p_qhdr, p_qout, p_qcut;
	i32 qtrack_w = 0;                                    // window length (0: none; a clone starts without); independent of track_w
	size_t qtrack_zeroed = 0; bool qtrack_dirty = false; // entries of d_qbin known to be zero; a call that failed between COUNT and EMIT left counts behind
	// what growing buffers cost this context (dev_ensure / pin_ensure: hipMalloc, hipHostMalloc, the frees and the quiesce in front of them) -- gsa_get_alloc_stats
	double alloc_ms = 0; long long alloc_n = 0, alloc_bytes = 0;
};

// Every DevBuf member above and in QuerySlot, once: GSA_DEVBUFS the device buffers (gsa_destroy frees them with hipFree, gsa_debug_buffers lists them), GSA_PINBUFS the pinned
// host buffers (hipHostFree).  A member missing here leaks with every context: tests/test_build_checks.py holds the two lists against the declarations.
#define GSA_DEVBUFS(X) \
	X(d_bwt) X(d_bwt_ref) X(d_occ_base) X(d_sa) X(d_ref) X(d_chr_end) X(d_chr_of_end) X(qs[0].d_query) X(qs[1].d_query) X(qs[0].d_bndtab) X(qs[1].d_bndtab) \
	X(tmp) X(d_cnt) X(d_zero) X(d_mail) X(d_lb_status[0]) X(d_lb_status[1]) X(d_sa_dense) X(d_kmer) X(d_kmer_lo) X(d_pres) X(d_ref2) \
	X(d_cand_s) X(d_cand_len) X(d_cand_x0) X(d_cand_freq) X(d_onpath) X(d_cand_cnt) X(d_heavy) X(dn_lf) X(dn_x0) X(d_chunk_hits) X(d_chunk_base) \
	X(d_key_a) X(d_key_b) X(d_val_a) X(d_val_b) X(s_q) X(s_len) X(s_r) X(s_gid) X(d_flag) X(d_scan) X(g_beg) X(w_j0) X(d_pdbm) X(d_pdby) X(d_pdcb) X(d_gpre) X(d_key_c) X(d_val_c) \
	X(a_q) X(a_len) X(a_r) X(a_gb) X(a_ge) X(a_uniq) X(a_cu) X(a_alive) X(a_ws) X(a_wid) X(a_next) X(a_brk) X(a_aurank) X(a_aulist) X(a_runinfo) X(w_best) X(w_sum) X(w_n) \
	X(d_btab) X(d_flag2) X(d_scan2) X(d_i64a) X(b_q) X(b_len) X(b_r) X(b_gb) X(b_ge) X(c_q) X(c_len) X(c_r) X(c_gb) X(c_ge) X(c_bid) X(blk_beg) X(blk_end) X(blk_score) \
	X(r_q) X(r_len) X(r_r) X(r_bid) X(r_tmp_q) X(r_tmp_len) X(r_tmp_r) X(r_tmp_bid) X(r_cut4) X(r_cut5) X(r_simjob) X(r_simres) X(d_leaf) \
	X(fb_seedbase) X(fb_sbeg) X(fb_fragbase) X(f_rec) X(f_rec16) X(f_type) X(f_mism) X(f_alnlen) X(f_job) X(f_score) \
	X(d_dp_lane_order) X(d_dp_bnd) X(d_dp_ctr) X(d_dp_jobs) X(d_dp_large) X(d_tail) X(d_band_dir) X(d_band_seq) X(d_band_cert) X(d_band_stat) \
	X(e_id) X(e_rec) X(e_list) X(e_off1) X(e_off2) X(e_opsoff) X(e_nops) X(e_ops) X(e_rev) X(r_head) X(f_early) X(r_orig) X(r_tmp_orig) \
	X(j_frag) X(j_opsoff) X(j_nops) X(d_ops) X(j_cells) X(d_alnoff) X(bl_alnlen) X(bl_score) X(d_bblk) X(d_dp_arena) \
	X(d_vblk) X(d_vcnt) X(d_vwg) X(d_var) X(d_cblk) X(d_cout) X(d_ccnt) X(d_cwg) X(d_cpre) X(d_crun) X(d_cops) X(d_crpos) X(d_cqpos) X(d_slen) X(d_swg) X(d_spre) X(d_sout) X(d_cs) \
	X(d_lpos) X(d_lblk) X(d_lpick) X(d_lwg) X(d_lhit) X(d_tblk) X(d_tiv) X(d_tbin) X(d_twg) X(d_tout) X(d_sgwg) X(d_sgpre) X(d_sgbnd) X(d_sgout) X(d_sgseg) X(d_pblk) X(d_ppre) X(d_pwg) X(d_pstage) X(d_rgpos) X(d_rgpre) X(d_rgwg) X(d_rghit) X(d_qblk) X(d_qiv) X(d_qbin) X(d_qwg) X(d_qout) X(d_qcut) \
	X(leaf[0]) X(leaf[1]) X(leaf[2]) X(leaf[3]) X(leaf[4]) X(leaf[5]) X(leaf[6]) X(leaf[7]) X(leaf[8])
#define GSA_PINBUFS(X) \
	X(p_frags) X(p_tail) X(p_leaf) X(p_blk) X(p_dp) X(p_sj) X(p_sj_early) X(p_jpatch) X(p_early) X(qs[0].p_bndtab) X(qs[1].p_bndtab) X(p_bblk) X(p_ba0) \
	X(p_vblk) X(p_vhdr) X(p_var) X(p_cblk) X(p_chdr) X(p_cout) X(p_cops) X(p_shdr) X(p_sout) X(p_cs) X(p_lblk) X(p_lhdr) X(p_lhit) X(p_tblk) X(p_tiv) X(p_thdr) X(p_tout) X(p_sghdr) X(p_sgout) X(p_sgseg) X(p_pblk) X(p_phdr) X(p_pstage) X(p_rghdr) X(p_rghit) X(p_qblk) X(p_qiv) X(p_qhdr) X(p_qout) X(p_qcut)

// A buffer is about to be freed: nothing of this context may still use it -- not only the main stream: the early striped DP launch runs on
// stream_aux[0] beside stages 3-7 and shares direction / boundary / ticket buffers with the late launch, strings and record copies run on
// stream_aux[1] / [2].  (Until round 4 only the main stream was waited for: a late launch that outgrew a shared buffer while the early one
// was still running freed it under the kernel -- a rare "memory access fault", seen once in a four-context run.)
static inline void ctx_quiesce(gsa_ctx *c)
{
	hipStreamSynchronize(c->stream);
	for (int i = 0; i < 4; i++) if (c->stream_aux[i]) hipStreamSynchronize(c->stream_aux[i]);
}

void *dev_take_reserved(int device, size_t bytes, size_t *got);   // gsa_create.hip  (gsa_reserve_index: memory set aside for the dense SA / the k-mer table)
// exact = true: the index tables -- asked for once, never grown: no slack (the dense SA of a human index is 49 GB: half again was 25 GB of HBM and 0.1 s of gsa_create)
template <class T> static inline T *dev_ensure(gsa_ctx *c, DevBuf &b, size_t n, bool exact = false)
{
	size_t bytes = (n ? n : 1) * sizeof(T);
	b.len = bytes;
	if (bytes <= b.cap) return (T *)b.p;
	const auto t0_ = std::chrono::steady_clock::now();
	if (b.p) { ctx_quiesce(c); hipFree(b.p); b.p = nullptr; b.cap = 0; }
	size_t want = exact ? bytes + 256 : bytes + bytes / 2 + 256;      // (half again: a context that meets a somewhat larger contig or bundle than it has seen does not stop to reallocate)
	if (exact && bytes >= ((size_t)1 << 30)) { size_t got = 0; if (void *r = dev_take_reserved(c->device, want, &got)) { b.p = r; b.cap = got; return (T *)b.p; } }
	if (hipMalloc(&b.p, want) != hipSuccess) { gsa_fail(c, GSA_ERR_NOMEM, "hipMalloc"); return nullptr; }
	b.cap = want;
	c->alloc_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0_).count(); c->alloc_n++; c->alloc_bytes += (long long)want;
	return (T *)b.p;
}
// inside a stage driver (`c` is the context, the function returns an error code): c->buf holds n elements of T, or the driver fails
#define ENS(T, buf, n) do { if (!dev_ensure<T>(c, c->buf, (size_t)(n))) return GSA_ERR_NOMEM; } while (0)

template <class T> static inline T *pin_ensure(gsa_ctx *c, DevBuf &b, size_t n)
{
	size_t bytes = (n ? n : 1) * sizeof(T);
	if (bytes <= b.cap) return (T *)b.p;
	const auto t0_ = std::chrono::steady_clock::now();
	if (b.p) { ctx_quiesce(c); hipHostFree(b.p); b.p = nullptr; b.cap = 0; }
	size_t want = bytes + bytes / 4 + 4096;
	if (hipHostMalloc(&b.p, want) != hipSuccess) { gsa_fail(c, GSA_ERR_NOMEM, "hipHostMalloc"); return nullptr; }
	b.cap = want;
	c->alloc_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0_).count(); c->alloc_n++; c->alloc_bytes += (long long)want;
	return (T *)b.p;
}

// stage drivers (one per translation unit)
int build_dense_sa(gsa_ctx *c, u64 n_sa);   // k_tables.hip  (gsa_create_opts: build_ref2, densify_sa, build_kmer_table)
int build_ref2(gsa_ctx *c);                 // k_tables.hip  (the 2-bit copy of RefSequence)
int densify_sa(gsa_ctx *c, u64 n_sa);       // k_tables.hip  (the dense SA by LF walks from the samples)
int build_kmer_table(gsa_ctx *c);           // k_tables.hip  (needs the Occ blocks and the dense SA; its size comes from the free device memory)
int unpack_pac(gsa_ctx *c, const uint8_t *d_pac, i64 G, uint8_t *d_ref);   // k_tables.hip  (GSA_CREATE_REF_PAC: RefSequence from the .pac bytes, on the device)
int build_occ(gsa_ctx *c, const void *ref_layout, u64 n_blocks128);   // k_tables.hip: the device's Occ blocks from the reference's layout
int build_presence(gsa_ctx *c);             // k_tables.hip  (after MinSeedLength changed)
struct IxOpts { bool wide; i64 batch_cap, occ_segment, active_cap; };      // which sorter of the device index builder; the wide one's caps (0: the default)
struct IxStats { double ms = 0; i32 rounds = 0; i64 batches = 0, active = 0; u64 peak = 0; };
int build_tables_from_pac(gsa_ctx *c, const uint8_t *pac, i64 G, const IxOpts &o);   // k_index.hip  (gsa_create_from_pac: Occ blocks, both SAs and RefSequence from the suffix sort -- narrow, or the batched 64-bit one: GSA_CREATE_SORT_WIDE -- nothing copied home)
int stage1_seed(gsa_ctx *c);          // k_seed.hip
int stage1_dense(gsa_ctx *c, hipStream_t st, const uint8_t *d_q, i32 qlen, i64 n_chunks, u64 n_heavy, bool dense_all, bool sweep_all, size_t ccap, u64 &hits, u64 &maxcand, u64 &occ_all);   // k_seed_dense.hip  (stage1_seed's dense kernels: launch, wait, counters)
int prepare_pd_bitmap(gsa_ctx *c, i64 n_hits, i64 n_chunks = 0);   // k_seed_select.hip  (whether this contig keeps the bitmap of occupied PosDiff values, cleared)
int stage1_select(gsa_ctx *c, i64 n_chunks, i64 n_hits, size_t ccap, u64 contig_maxcand, i32 s_off, u64 occ_all);   // k_seed_select.hip  (stage1_seed's tail: hits located and keyed, groups)
int stage1_import_hits(gsa_ctx *c, const u64 *keys, const u32 *vals, i64 n);   // k_seed_select.hip
int stage1_finish_split(gsa_ctx *c);  // k_seed_select.hip
int stage1_restore_pdbm(gsa_ctx *c);  // k_seed_select.hip  (the PosDiff bitmap again from the hits a finished stage 2 left in d_key_a)
int seed_view_sort(gsa_ctx *c);       // k_seed_select.hip  (PosDiff-sorted seeds + groups: stage-1 view, or front of stage 2 without the PosDiff bitmap)
int stage2_chain(gsa_ctx *c);         // k_chain.hip
int launch_early_dp(gsa_ctx *c);      // k_chain.hip  (striped DP for the large gaps listed at the end of stage 2)
int stage2_fetch_host(gsa_ctx *c);    // k_chain.hip  (counts + S2 block table for the stage-2 view)
void collect_events(gsa_ctx *c);      // gsa_api.hip  (deferred hipEventElapsedTime of stages 1-2)
int stage345_refine(gsa_ctx *c);      // k_refine.hip  (device part of S3, S4, S5 + leaf table)
int stage7_fill(gsa_ctx *c);          // k_extend.hip  (S6: gap records of the final block list)
i64 frags_count(gsa_ctx *c);          // k_extend.hip  (record count, fetched from the mailbox when still unknown)
int stage78_extend(gsa_ctx *c);       // k_extend.hip  (S7: classification, DP, gapped strings, block sums)
int run_gapsim_jobs(gsa_ctx *c, i32 n, const i32 *d_n, const i32 *d_q1, const i32 *d_q2, const i64 *d_r1, const i64 *d_r2, i32 *d_res, const i32 *d_jseed, i32 *d_cut4);   // k_gapsim.hip
void dp_count_cells(gsa_ctx *c, i32 n_ub, const i32 *len1, const i32 *len2, hipStream_t stream);   // k_dp.hip (profiling)
// the passes over a stage-8 result (shared parts: gsa_walk.h).  `out` comes in zeroed (gsa_api.hip's exports do that, once) and is written only on success
int call_variants(gsa_ctx *c, i32 k, gsa_variants *out);   // k_variants.hip  (VariantIdentification over the stage-8 result of contig k)
int block_cigars(gsa_ctx *c, i32 k, gsa_cigars *out, bool pos = false);      // k_cigar.hip  (the CIGAR of every block of the stage-8 result of contig k; pos: the runs' first positions too, into d_crpos / d_cqpos)
int block_cs(gsa_ctx *c, i32 k, gsa_cs *out, gsa_cigars *cig_out = nullptr);   // k_cs.hip  (the cs string of every block: the CIGAR pass with positions, then its own three passes; cig_out: that CIGAR pass's answer)
int lift_positions(gsa_ctx *c, i32 k, gsa_lifts *out);      // k_lift.hip  (the positions of gsa_lift_set through the stage-8 result of contig k)
int block_segs(gsa_ctx *c, i32 k, gsa_segs *out, gsa_cigars *cig_out = nullptr, const gsa_cigars *have = nullptr);   // k_segs.hip  (the chain triples of every block: the CIGAR pass with positions -- or, have: the one that has just run for this contig -- then four launches per run / per segment)
int ref_track(gsa_ctx *c, i32 k, gsa_tracks *out);          // k_track.hip  (the per-window track of the stage-8 result of contig k at the window of gsa_track_set)
int lift_regions(gsa_ctx *c, i32 k, gsa_region_lifts *out);   // k_regions.hip  (the regions of gsa_regions_set through the stage-8 result of contig k)
int query_track(gsa_ctx *c, i32 k, gsa_qtracks *out);       // k_qtrack.hip  (the per-window track of the stage-8 result of contig k over the query contig, at the window of gsa_qtrack_set)
int project_blocks(gsa_ctx *c, i32 k, gsa_proj_stat *out);   // k_proj.hip  (the blocks of contig k painted into the context's accumulator)
int proj_open(gsa_ctx *c, gsa_ctx *share, u32 flags);       // k_proj.hip  (gsa_proj_open / close / clear / fetch / merge behind their argument checks)
int proj_release(gsa_ctx *c);                               // k_proj.hip  (gsa_proj_close, gsa_destroy: the context's reference dropped, the array freed with the last one)
int proj_clear(gsa_ctx *c);
int proj_fetch(gsa_ctx *c, i64 p0, i64 n, char *text, u32 *words);
int proj_merge(gsa_ctx *c, i64 p0, i64 n, const u32 *words);
int build_index_device(gsa_ctx *c, const uint8_t *pac, i64 G, const IxOpts &o, const char *who, u64 *primary, u64 L2[5], u32 *bwt, u64 *sa, IxStats *out);   // k_index.hip  (suffix sort -- narrow, or k_index_wide.hip's above 2^31 - 2 suffixes -- + BWT / Occ / SA samples of forward + reverse complement)
int host_stage4_5_6(gsa_ctx *c, int stage);    // gsa_blocks.cpp
int host_stage8_finish(gsa_ctx *c);            // gsa_blocks.cpp
int build_block_view(gsa_ctx *c);              // gsa_blocks.cpp
void bundle_split_lists(gsa_ctx *c);           // gsa_blocks.cpp  (a bundle of contigs: one AlnBlockVec per contig for stages 4-6 ...
void bundle_join_lists(gsa_ctx *c);            // gsa_blocks.cpp   ... joined again, contig after contig, for stages 7-8)
// the host side of the C ABI, file to file
#define GSA_BUNDLE_MAX_CONTIGS 4096
int reset_run_state(gsa_ctx *c);      // gsa_query.hip  (back to stage 0: nothing of the previous run in flight or half-consumed; the query, its geometry and `bnd` stay)
int set_query_bundle(gsa_ctx *c, const char *const *query, const int32_t *qlen, int32_t n, bool dev_q);   // gsa_query.hip  (gsa_align_bundle's gsa_set_query)
// (the exports gsa_align_many_ex calls too; all of them: result_pass in gsa_api.hip)
int lift_call(gsa_ctx *c, int32_t k, gsa_lifts *out);   // gsa_api.hip  (gsa_lift)
int track_call(gsa_ctx *c, int32_t k, gsa_tracks *out);   // gsa_api.hip  (gsa_ref_track)
int qtrack_call(gsa_ctx *c, int32_t k, gsa_qtracks *out);   // gsa_api.hip  (gsa_query_track)
int proj_call(gsa_ctx *c, int32_t k, gsa_proj_stat *out);   // gsa_api.hip  (gsa_project)
int regions_call(gsa_ctx *c, int32_t k, gsa_region_lifts *out);   // gsa_api.hip  (gsa_lift_regions)
int segs_call(gsa_ctx *c, int32_t k, gsa_segs *out, gsa_cigars *cig, const gsa_cigars *have);   // gsa_api.hip  (gsa_block_segs; cig / have: as block_segs, for gsa_align_many_ex)
int cs_call(gsa_ctx *c, int32_t k, gsa_cs *out, gsa_cigars *cig);   // gsa_api.hip  (gsa_block_cs; cig: the CIGARs the pass computed on its way, for gsa_align_many_ex)
struct LgJob { i32 job, m, n; };
int launch_stripes(gsa_ctx *c, hipStream_t ss, std::vector<LgJob> &large, const uint8_t *pool1, const i64 *off1, const uint8_t *pool2, const i64 *off2,
                   uint8_t *ops, const i64 *ops_off, i32 *ops_len, uint8_t *rev, int err_slot);   // k_dp_stripe.hip
// the band class of a striped batch (k_dp_band.hip): large[idx[k]] are its jobs, in the order of their certified flags cert[k] (the returned array: == tag where job k's result stands)
struct BandJob { i32 job, m, n, base; i64 diroff, seqoff; };      // base: diagonal i - j of lane 0's even diagonal; seqoff: the pair's code strings (in X's entry)
bool dp_band_eligible(const gsa_ctx *c, int m, int n, i64 stripe_steps);
size_t dp_band_table_bytes(size_t njobs);
int launch_band(gsa_ctx *c, hipStream_t st, const std::vector<LgJob> &large, const std::vector<i32> &idx, BandJob *tab, const uint8_t *pool1, const i64 *off1, const uint8_t *pool2, const i64 *off2,
                uint8_t *ops, const i64 *ops_off, i32 *ops_len, uint8_t *rev, const u32 **cert, u32 *tag);
int launch_small_dp(gsa_ctx *c, hipStream_t st, i32 nlane, const i32 *order_lane, i32 nsmall, const i32 *order_small, const uint8_t *pool1, const i64 *off1, const i32 *len1,
                    const uint8_t *pool2, const i64 *off2, const i32 *len2, uint8_t *ops, const i64 *ops_off, i32 *ops_len, const i32 *jfrag, gsa_frag *frag);   // k_dp_small.hip  (k_dp_lane + k_dp_small beside `st`; ev[12] marks their end)
struct Ksw2Launch { i32 n = 0, nsmall = 0, nlarge = 0; bool small_in_flight = false; };      // what run_ksw2_jobs left running
int run_ksw2_jobs(gsa_ctx *c, i32 n_ub, const uint8_t *pool1, const i64 *off1, const i32 *len1,
                  const uint8_t *pool2, const i64 *off2, const i32 *len2, uint8_t *ops, const i64 *ops_off, i32 *ops_len, i64 ops_total, Ksw2Launch *out,
                  const i32 *jfrag = nullptr, gsa_frag *frag = nullptr, bool mail_clean = false);   // k_dp.hip  (jfrag/frag: the small kernels also set aln_len of the job's record;
                  // mail_clean: the caller's last pass already zeroed mail[M_DPERR .. M_DPERR + 7])

#endif
