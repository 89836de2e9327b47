/* include/gsa_hip.h -- C ABI of libgsa_hip.so, the MI355X (gfx950) hot path of a
 * GSAlign-compatible whole-genome aligner.
 *
 * The reference (hsinnan75/GSAlign v1.0.22) has no plugin / FFI interface; its
 * hot path is the set of functions GenomeComparison() launches per query contig
 * (reference src/GSAlign.cpp:483-540) and they communicate through globals.
 * This header is the seam a maintainer would bind instead (SURVEY.md section
 * 8(b)); every entry point cites the reference code it replaces.  Plain C:
 * pointers and sizes only, no C++/torch types.  One gsa_ctx per GPU; a context
 * is not thread-safe; calls are synchronous for the caller.
 *
 * All results are bit-identical to the reference's: seeds, blocks, gap records,
 * op strings, scores.
 */
#ifndef GSA_HIP_H
#define GSA_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct gsa_ctx gsa_ctx;

/* error codes (negative); gsa_last_error() has the text */
enum {
	GSA_OK = 0,
	GSA_ERR_ARG = -1,      /* bad argument                      */
	GSA_ERR_HIP = -2,      /* a HIP runtime call failed         */
	GSA_ERR_NOMEM = -3,    /* device or host allocation failed  */
	GSA_ERR_STATE = -4,    /* call order violated               */
	GSA_ERR_LIMIT = -5     /* an internal capacity was exceeded */
};

/* The in-memory index the reference keeps in Refbwt / RefSequence / ChromosomeVec
 * (structure.h:28-38,141-155; filled by bwa_idx_load + RestoreReferenceInfo,
 * bwt_index.cpp:147-264).  Host pointers; gsa_create copies them to the device
 * and does not keep them. */
typedef struct {
	uint64_t primary;          /* bwt_t::primary                                        */
	uint64_t L2[5];            /* bwt_t::L2, L2[0] = 0, L2[4] = seq_len = 2G            */
	const uint32_t *bwt;       /* bwt_t::bwt: interleaved Occ checkpoints + 2-bit BWT   */
	uint64_t bwt_words;        /* bwt_t::bwt_size                                       */
	const uint64_t *sa;        /* bwt_t::sa, sa[0] = (uint64_t)-1, sa_intv = 32         */
	uint64_t n_sa;             /* bwt_t::n_sa                                           */
	const char *ref;           /* RefSequence: 2G ASCII bytes, forward + reverse compl. */
	int64_t G;                 /* GenomeSize (forward length)                           */
	const int32_t *chr_len;    /* ChromosomeVec[i].len                                  */
	int32_t n_chr;             /* iChromsomeNum                                         */
} gsa_index_view;

/* The tunables the reference parses into globals (main.cpp:202-214,236-299,323). */
typedef struct {
	int32_t min_seed_len;      /* -slen  MinSeedLength     [15]; forced to 10 by -sen  */
	int32_t max_indel;         /* -ind   MaxIndelSize      [25]                        */
	int32_t min_block_score;   /* -clr   MinAlnBlockScore  [200] (50 with -sen)        */
	int32_t min_aln_len;       /* -alen  MinAlnLength      [200]                       */
	int32_t min_identity;      /* -idy   MinSeqIdy         [70]                        */
	int32_t sensitive;         /* -sen   bSensitive        [0]                         */
	int32_t one_on_one;        /* -one   OneOnOneMode      [0]                         */
} gsa_params;
void gsa_default_params(gsa_params *p);

/* ---- records ------------------------------------------------------------ */
/* one located exact match; the reference's FragPair_t with bSeed = true
 * (structure.h:103-113), order = CompByPosDiff (ProcessCandidateAlignment.cpp:3-7) */
typedef struct { int32_t qpos; int32_t len; int64_t rpos; } gsa_seed;

/* FragPair_t of a finished block (structure.h:103-113), expanded.  aln_off/aln_len address the two gapped strings of a
 * non-seed pair inside gsa_result::aln1 / aln2.  This is the VIEW type: results travel as the 16-byte gsa_rec defined below and are expanded
 * with gsa_rec_expand / gsa_expand_frags where a consumer wants FragPair_t-shaped records. */
typedef struct {
	int32_t bseed, qpos, qlen, rlen;
	int64_t rpos;
	int64_t aln_off;
	int32_t aln_len;
	int32_t _pad;
} gsa_frag;

/* The record as it crosses PCIe: 16 bytes instead of gsa_frag's 40; a 250 Mb contig at 1 % divergence has 4.1 M
 * records.  FillAlnBlockGaps / IdentifyNormalPairs (ProcessCandidateAlignment.cpp:241-276) put at most ONE gap pair
 * between two consecutive seeds, and it starts where the seed in front of it ends -- so a block's records are
 * seed [gap] seed [gap] ... seed, a seed needs (qPos, len, rPos), and a gap only its two lengths and its string:
 * its positions are those of the record in front of it.  w0 >= 0: seed {qpos, len, rpos}; w0 < 0: gap
 * {-1 - qlen, rlen, aln_len, aln_off} (string offsets fit 32 bits: GSA_ERR_LIMIT guards that per contig). */
typedef union {
	struct { int32_t qpos, len; int64_t rpos; } seed;
	struct { int32_t nqlen, rlen, aln_len; uint32_t aln_off; } gap;
} gsa_rec;

static inline int gsa_rec_is_seed(const gsa_rec *r) { return r->seed.qpos >= 0; }
/* record i of `recs` as a FragPair_t (a gap reads the seed in front of it: i > 0 then, by construction) */
static inline void gsa_rec_expand(const gsa_rec *recs, int64_t i, gsa_frag *f)
{
	const gsa_rec *r = recs + i;
	if (r->seed.qpos >= 0) {
		f->bseed = 1; f->qpos = r->seed.qpos; f->qlen = f->rlen = r->seed.len; f->rpos = r->seed.rpos; f->aln_off = 0; f->aln_len = 0;
	} else {
		const gsa_rec *s = r - 1;
		f->bseed = 0; f->qpos = s->seed.qpos + s->seed.len; f->rpos = s->seed.rpos + s->seed.len;
		f->qlen = -1 - r->gap.nqlen; f->rlen = r->gap.rlen; f->aln_off = (int64_t)r->gap.aln_off; f->aln_len = r->gap.aln_len;
	}
	f->_pad = 0;
}
static inline void gsa_expand_frags(const gsa_rec *recs, int64_t n, gsa_frag *out)
{
	for (int64_t i = 0; i < n; i++) gsa_rec_expand(recs, i, out + i);
}

/* AlnBlock_t (structure.h:115-122) after the identity filter (GSAlign.cpp:529-540) */
typedef struct {
	int32_t score, aln_len, bdup, n_frag;
	int64_t frag_off;          /* first record of this block             */
	int32_t bdir, gpos, chr;   /* Coordinate_t from GenCoordinateInfo    */
	int32_t _pad;
} gsa_block;

/* everything GenomeComparison() leaves in AlnBlockVec for one query contig,
 * in the reference's order (RemoveBadAlnBlocks, GSAlign.cpp:540).  Memory is
 * owned by the context and valid until the next gsa_align_contig/gsa_destroy. */
typedef struct {
	int32_t n_blocks;
	int64_t n_frags;
	int64_t n_aln;
	const gsa_block *blocks;
	const gsa_rec *recs;       /* n_frags compact records, block after block (gsa_block::frag_off / n_frag) */
	const char *aln1, *aln2;   /* reference-side / query-side gapped strings */
} gsa_result;

/* ---- life cycle --------------------------------------------------------- */
int  gsa_create(int device, const gsa_index_view *idx, const gsa_params *prm, gsa_ctx **out);
/* gsa_create with layout options.  GSA_CREATE_WIDE: the device layout of a text with >= 2^32 BWT rows (64-bit dense SA,
 * 32-byte k-mer entries) whatever the text length -- what a full human index (bwt_t::seq_len = 6.2 G, structure.h:28-38)
 * gets by itself; on a small index it lets the tests drive that code path. */
#define GSA_CREATE_WIDE 1u
/* GSA_CREATE_KMER_K(k), 2 <= k <= 15: the jump table that replaces the first k steps of BWT_Search (bwt_search.cpp:152-165) is built for
 * k-mers of this length if it fits (default: by text length and free device memory; tests: a long table on a short text). */
#define GSA_CREATE_KMER_K(k) (((uint32_t)(k) & 15u) << 8)
/* GSA_CREATE_PRIO(mode), mode 1..3: stream priorities for a host that drives SEVERAL contexts on one GPU (clones inherit it).  The short bookkeeping passes of
 * chaining / refinement / extension run on a stream of the greatest priority, the seed-search kernels on a stream of their own (1, 3: normal priority, 2: least),
 * the striped DP normal (3: least).  Results do not depend on it.  0 (default): every stream at the default priority. */
#define GSA_CREATE_PRIO(mode) (((uint32_t)(mode) & 3u) << 16)
/* GSA_CREATE_REF_PAC: idx->ref points at the bytes of the .pac file (G bases, four per byte, as bns_fasta2bntseq wrote them: bntseq.c:110-211) instead of at RefSequence.
 * The reference unpacks .pac into 2G ASCII bytes on the host (RestoreReferenceInfo, bwt_index.cpp:229-264) before anything else can start; with this flag the device does
 * that loop itself -- G / 4 bytes cross PCIe instead of 2G, and a host program can unpack its own copy (for its emitters) WHILE gsa_create builds the device tables. */
#define GSA_CREATE_REF_PAC 4u
/* GSA_CREATE_SORT_WIDE (gsa_create_from_pac only): the suffixes are sorted by the wide device builder (gsa_build_index_opts, GSA_BUILD_WIDE) whatever the
 * text length, and its 64-bit suffix array becomes the wide dense SA -- GSA_CREATE_WIDE is implied.  This is how a reference over 1 073 741 822 bases gets a
 * context from its sequence; under that length it lets the tests drive the wide builder (its batch cap and Occ segment: gsa_set_index_build_caps). */
#define GSA_CREATE_SORT_WIDE 2u
int  gsa_create_opts(int device, const gsa_index_view *idx, const gsa_params *prm, uint32_t flags, gsa_ctx **out);
/* A context from the reference SEQUENCE instead of from its index files: what bwa_idx_build (BWT_Index/bwtindex.c:77-149) followed by bwa_idx_load +
 * RestoreReferenceInfo (bwt_index.cpp:147-264) amount to, with no file and no host array in between.  pac = ceil(G / 4) host bytes as gsa_build_index takes them;
 * chr_len / n_chr / prm as in gsa_index_view / gsa_create; flags as for gsa_create_opts (GSA_CREATE_REF_PAC is implied and accepted).  The device sorts the 2G + 1
 * suffixes (gsa_build_index's sorter), and its suffix array becomes the context's dense SA; Occ blocks, SA samples, both text forms and the k-mer tables follow on
 * the device.  The context is the one gsa_create_opts makes from the index files of the same sequence -- the same device tables bit for bit -- and is cloned
 * (gsa_clone, gsa_clone_to_device) and destroyed like it.  A reservation of gsa_reserve_index on `device` is released, not adopted.
 * Errors in this order: NULL pointers, G <= 0, n_chr <= 0, sum(chr_len) != G, an unknown flag GSA_ERR_ARG; G > 1 073 741 822 GSA_ERR_LIMIT (before anything is
 * allocated and before pac is read; with GSA_CREATE_SORT_WIDE the bound is gsa_build_index_opts's, 4 294 967 295); no device GSA_ERR_HIP; ~52 bytes of device memory per suffix that are not there GSA_ERR_NOMEM.  gsa_last_error(NULL) has the text. */
int  gsa_create_from_pac(int device, const uint8_t *pac, int64_t G, const int32_t *chr_len, int32_t n_chr, const gsa_params *prm, uint32_t flags, gsa_ctx **out);
/* Test support: device table `which` of a context (its own, or the one it borrows) copied to dst[cap]; *bytes = its size, dst == NULL only reports it; an absent
 * table reports 0.  Only the DEFINED extent of a table is exported: the dense SA seq_len + 1 entries, the Occ blocks the 2 x n_blocks uint4 that were written,
 * ref2 the packed words.  GSA_TABLE_HEADER: 48 bytes {primary, L2[5]}. */
enum { GSA_TABLE_HEADER = 0, GSA_TABLE_OCC = 1, GSA_TABLE_OCC_BASE = 2, GSA_TABLE_SA_DENSE = 3, GSA_TABLE_SA = 4, GSA_TABLE_KMER = 5, GSA_TABLE_KMER_LO = 6,
       GSA_TABLE_PRES = 7, GSA_TABLE_REF = 8, GSA_TABLE_REF2 = 9 };
int  gsa_export_index_table(gsa_ctx *ctx, int which, void *dst, uint64_t cap, uint64_t *bytes);
/* Optional, before gsa_create: sets device memory aside for the two largest device tables of an index whose text has `seq_len` BWT rows (bwt_t::seq_len, the fifth
 * word of the .bwt header: structure.h:28-38) -- the dense suffix array and the k-mer table, 84 GB for a human index, ~0.4 s of hipMalloc -- so that a host can do that
 * while it is still READING the index files (the reference's bwa_idx_load reads first and allocates as it goes, bwt_index.cpp:147-227).  `flags` as for gsa_create_opts.
 * The next gsa_create[_opts] on `device` adopts what fits and frees the rest; gsa_release_reserved frees a reservation nobody adopted.  Thread-safe. */
int  gsa_reserve_index(int device, uint64_t seq_len, uint32_t flags);
void gsa_release_reserved(int device);
/* Tunables that are not aligner parameters (the library reads no environment variable).  A clone starts with its parent's values;
 * gsa_align_many takes its policy from ctx[0].
 *   "split_min"      bases; gsa_align_many seeds a contig of at least this length on several contexts when contexts would idle (20 000 000)
 *   "bundle_contig"  bases; contigs up to this length share passes (16 000 000; 0 = never)      "bundle_cap"  bases per bundle, about (64 000 000)
 *   "seed_budget"    wave-iterations a 10 000-bp chunk may take in the speculative seed kernel before the dense kernels redo it (256)
 *   "dp_lane"        cells; gap alignments up to this size run one per lane (512; 0 = no lane class: every gap alignment below the striped kernel runs one per wavefront)
 *   "seed_mode"      1 = speculative kernel + dense kernels for the chunks it gives up on (default), 0 = every chunk through the
 *                    right-to-left sweep, 2 = one search per start instead of the sweep
 *   "pd_bitmap"      0 = seed groups by the PosDiff sort (SeedGrouping as written, GSAlign.cpp:126-143) even where the bitmap scan applies
 *   "sweep_shape"    launch shape of the repeat-regime seed kernel (k_dense_sweep): -1 (default) by the number of dense chunks, 0 = four chunks per
 *                    workgroup and 160-start segments (many chunks), 1 = one chunk per workgroup and 40-start segments (few).  Results do not depend on it
 *   "dp_side"        1 = the striped DP launches its lower size class on a stream of its own, beside the upper class, instead of behind it (measured: the DP
 *                    span of a 250 Mb contig 4.9 -> 1.9 ms, but the refinement passes beside it starve: contig latency 13.7 -> 14.3 ms, throughput -4 % / +4 %); default 0
 *   "dp_pair"        the striped DP puts two jobs of a size class side by side into the 16-bit halves of a wavefront: 1 (default) = where that costs fewer
 *                    wave-steps than the two jobs one after the other and the class holds at least 4096 jobs (shorter lists are bound by their longest
 *                    job, not by instructions), 0 = never, 2 = every two neighbours, 3 = by the step count alone (2, 3: tests).  Results do not depend on it
 *   "dp_band"        near-diagonal jobs of the striped DP are first evaluated inside a band of diagonals, two jobs per wavefront, a step per anti-diagonal
 *                    (m + n steps instead of (m + 63) per 64 columns); a job whose band score proves the band exact keeps that result, any other runs in the
 *                    striped kernel as before: 1 (default) = jobs whose band costs at most 3/4 of the striped wave-steps, 0 = never, 2 = every job the
 *                    layout admits (tests).  "dp_band_margin" B (32; 1 .. 63): the band is the diagonals from min(0, n - m) - B to max(0, n - m) + B and
 *                    must fit 128 diagonals.  Results do not depend on either
 *   "walk_chain_min" seeds; a contig with more seeds than this walks its window chain (chaining, GSAlign.cpp:326-338) in slices of the candidate list,
 *                    one launch (default 100 000; below that one workgroup holds the chain in LDS).  Results do not depend on it (tests: 0)
 *   "pd_two_level_min" blocks; PosDiff bitmaps larger than this are scanned in two passes (touched blocks listed, then counted); default 2 000 000
 *                    (references above ~1 Gbp).  "pres_from_kmer" 0 = the presence table always from a scan of the text.  Results do not depend on either
 *   "pd_bytes"       how k_seed_select marks the occupied PosDiff values of a contig whose hits scatter over the genome (-sen: thousands of chance hits per
 *                    10 000-bp chunk): 1 (default) = through a byte per value, plain stores, packed into the bitmap by a pass of its own, when there are at least
 *                    512 hits per chunk, at most 256 values per hit and at most 2^32 values (2 GB per context for a 64 Mb bundle against a 12 Mb reference); 0 = always with atomics
 *                    on the bitmap; 2 = always through the bytes (tests).  Results do not depend on it
 *   "seed_lhop"      test hook: entries of the seed kernel's long-hop table that a chunk may use (a power of two >= 16; 0 = all of them)
 *   "dp_safe", "dp_fake_timeout"   test hooks: one striped DP job per launch; the next n contigs report a stripe hand-off time-out once
 *   "dbg_dp_epoch", "dbg_band_epoch", "dbg_lb_epoch", "dbg_walk_epoch"   test hooks: set a launch epoch (gsa_get_launch_counters [2], [3], [0], [4]) once the
 *                    context's work in flight is through, so that the next launch is the one that comes round.  Forward only and inside the counter's width
 *                    (16, 32, 30, 32 bits): GSA_ERR_ARG otherwise -- the hook can make no stale word valid again
 *   "dbg_lb_ticket", "dbg_walk_ticket"   test hooks: set a ticket counter ([1], [5]), the host's value and the device word together; any 32-bit value.  The two
 *                    "walk" hooks: GSA_ERR_STATE before the context's first sliced chain walk (which starts both counters at zero)
 * Unknown names and values outside an option's range (negative sizes, seed_budget 0, ...): GSA_ERR_ARG, nothing changed.
 * Until round 4 some of these were environment variables read by the library (GSA_SPLIT_MIN, GSA_BUNDLE_CONTIG, GSA_BUNDLE_CAP, GSA_SEED_BUDGET,
 * GSA_DP_LANE, GSA_SEED_MODE, GSA_NO_PDBITMAP, GSA_FORCE_WIDE, GSA_KMER_K, GSA_DP_SAFE, GSA_DP_FAKE_TIMEOUT, GSA_NO_BIND): the library ignores
 * them now -- a C host sets the option (or the gsa_create_opts flag) itself; INTEGRATION.md lists the mapping. */
int  gsa_set_option(gsa_ctx *ctx, const char *name, int64_t value);
/* A further context on the same GPU that borrows `parent`'s device-resident index (read-only) and owns everything else.
 * The reference runs -t N threads inside one contig (GSAlign.cpp:477-526); contigs are independent (all per-contig state
 * is cleared at GSAlign.cpp:490), so a host drives N contexts from N threads on N contigs instead and the GPU overlaps
 * them.  Each context is single-threaded; `parent` must outlive its clones.  While clones of a context are alive,
 * gsa_set_params on THAT context may not change min_seed_len / sensitive (GSA_ERR_STATE: the clones read its presence bitmap
 * and short k-mer table); a clone may change its own parameters freely -- it then builds tables of its own. */
int  gsa_clone(gsa_ctx *parent, gsa_ctx **out);
/* A context on GPU `device` with a device index of ITS OWN, copied from `parent`'s device to device (over xGMI between GPUs) instead of
 * uploaded and rebuilt.  The reference loads its index once per process and every thread reads it (RefIdx / RefSequence / ChrLocMap,
 * bwt_index.cpp:147-264; the workers of GSAlign.cpp:477-526 share it); N GPUs need N copies, and gsa_create per GPU pays the PCIe upload
 * (10.7 GB for a human index) and the device-side table builds every time.  This pays one device-to-device copy of the finished tables.
 * The new context is independent of `parent` afterwards (it may outlive it), starts with parent's parameters and options, and may itself
 * be gsa_clone'd.  `device` may be parent's own GPU (a second, independent copy: what the tests on a one-GPU box exercise). */
int  gsa_clone_to_device(gsa_ctx *parent, int device, gsa_ctx **out);
void gsa_destroy(gsa_ctx *ctx);
/* Puts the CALLING host thread on the CPUs of the socket `device` hangs off (sysfs local_cpulist of its PCI function; a no-op
 * without that information).  The reference's worker threads (GSAlign.cpp:479, pthread_create) run
 * wherever the OS puts them, which costs nothing there; a thread that drives a GPU through ~60 short operations per 5 Mb
 * contig pays the inter-socket hop on every one (0.86 -> 0.65-0.75 ms per 5 Mb contig); chromosome-sized contigs ran 5 %
 * slower with bound threads, so nothing in the library calls this by itself: threads started by gsa_align_many inherit the
 * caller's affinity. */
int  gsa_bind_host_thread(int device);
/* Pinned host memory for query contigs (QueryChrVec[i].seq, main.cpp:82-114): the upload inside gsa_align_contig is then
 * one asynchronous DMA transfer.  Any other host memory works too (staged by the runtime). */
void *gsa_host_alloc(size_t bytes);
void  gsa_host_free(void *p);
/* The same for memory the host already owns (the std::string a FASTA loader filled): page-locks [p, p + bytes) in place so that the upload is a DMA
 * transfer instead of a staged copy (hipHostRegister: 10 ms per GB on the test host, hipHostMalloc of fresh pinned memory: 160 ms per GB).  The
 * reference keeps QueryChrVec[i].seq in ordinary memory (main.cpp:82-114); a host that does the same calls this once per sequence after loading.
 * Returns GSA_OK or GSA_ERR_HIP (then the buffer simply stays pageable). */
int   gsa_host_register(void *p, size_t bytes);
int   gsa_host_unregister(void *p);
int  gsa_set_params(gsa_ctx *ctx, const gsa_params *prm);
const char *gsa_last_error(gsa_ctx *ctx);   /* ctx may be NULL: error of the last failed gsa_create */

/* ---- the drop-in call ----------------------------------------------------
 * Replaces the body of the per-contig loop of GenomeComparison()
 * (GSAlign.cpp:483-540): S1 IdentifyLocalMEM ... S7 GenerateFragAlignment,
 * identity filter, GenCoordinateInfo, final RemoveBadAlnBlocks.
 * query = raw contig bytes exactly as loaded from FASTA (any case, IUPAC ok). */
int gsa_align_contig(gsa_ctx *ctx, const char *query, int32_t qlen, gsa_result *out);
/* The same with the contig ALREADY IN DEVICE MEMORY of the context's GPU (a loader that decodes FASTA on the GPU, or contigs
 * kept resident between runs): used in place, nothing crosses PCIe on the way in.  d_query: 16-byte aligned, qlen raw bytes
 * as above, valid and unmodified until the call returns.  gsa_device_alloc / gsa_device_upload / gsa_device_free are the
 * plain-C way to such a buffer for hosts that do not link a HIP runtime themselves. */
int gsa_align_contig_device(gsa_ctx *ctx, const char *d_query, int32_t qlen, gsa_result *out);
/* Upload of the NEXT contig while the current one is aligned.  The reference reads QueryChrVec[i].seq from host memory when the
 * loop reaches it (GSAlign.cpp:483-490, loader main.cpp:82-114); a GPU has to copy it first -- 4.8 ms per 250 Mb -- and that copy
 * hides behind the stages of the contig in front of it: a context has two device buffers for query sequences, gsa_prefetch_contig
 * (or _bundle) starts the copy of `query` into the one the next gsa_align_contig / gsa_align_bundle will not use and returns at
 * once; the following gsa_align_contig(ctx, query, qlen) -- same pointer, same length -- finds the contig on the device.  Call
 * order: gsa_prefetch_contig(next); gsa_align_contig(current); ...  `query` must stay valid and unmodified until it has been
 * aligned (or gsa_cancel_prefetch returned).  At most two contigs wait at a time (GSA_ERR_STATE beyond that).  After a prefetch
 * gsa_rewind may report GSA_ERR_STATE (the previous contig's device copy is gone).  gsa_align_many does all this by itself. */
int gsa_prefetch_contig(gsa_ctx *ctx, const char *query, int32_t qlen);
int gsa_prefetch_bundle(gsa_ctx *ctx, const char *const *query, const int32_t *qlen, int32_t n);
int gsa_cancel_prefetch(gsa_ctx *ctx);
void *gsa_device_alloc(int device, size_t bytes);
void  gsa_device_free(int device, void *p);
int   gsa_device_upload(int device, void *dst, const void *src, size_t bytes);

/* ---- the per-contig loop itself ------------------------------------------
 * Replaces the loop `for (QueryChrIdx = 0; QueryChrIdx < iQueryChrNum; ...)` of GenomeComparison() (GSAlign.cpp:483-548):
 * n contigs on n_ctx contexts -- contexts of different GPUs (gsa_create per device) and/or several contexts of one GPU
 * (gsa_clone) -- one host thread per context, contigs handed out longest first.  Contigs are independent in the
 * reference (all per-contig state is cleared at GSAlign.cpp:490), so results do not depend on n_ctx.
 * on_result(user, contig, res) is called by the worker that finished `contig`, possibly from several threads at once;
 * *res is valid during the callback only.  Returns the first error (the failing context holds the text). */
typedef int (*gsa_result_fn)(void *user, int32_t contig, const gsa_result *res);
#define GSA_MANY_IN_ORDER 1u   /* hand the contigs out in the order given (default: longest first) */
#define GSA_MANY_DEVICE   2u   /* query[] are device pointers (gsa_align_contig_device); all contexts on one GPU */
#define GSA_MANY_NO_SPLIT 4u   /* never seed one contig on several contexts (see below) */
#define GSA_MANY_NO_BUNDLE 8u  /* never align several short contigs in one pass (see gsa_align_bundle) */
#define GSA_MANY_NO_PREFETCH 16u /* upload every contig when its turn comes (default: a context uploads its next contig while it aligns the current one) */
/* With FEWER contigs than contexts (one chromosome, two GPUs: BASELINE configs[3]) the contexts are dealt out in groups, one
 * group per contig, sized by contig length, and a contig of at least 20 Mb (gsa_set_option "split_min") is seeded by chunk range on all
 * contexts of its group -- gsa_seed_chunks ... gsa_finish_contig below, driven from the library's own threads, hits moved
 * device to device (peer to peer between GPUs).  Results do not depend on the grouping. */
int gsa_align_many(gsa_ctx *const *ctx, int32_t n_ctx, const char *const *query, const int32_t *qlen, int32_t n,
                   uint32_t flags, gsa_result_fn on_result, void *user);

/* Several contigs in ONE pass.  The reference clears all per-sequence state between query sequences (GSAlign.cpp:483-490), so
 * contigs are independent; a short contig costs the GPU ~60 operations whatever its size, so short contigs are concatenated
 * (each padded with N to a 10 000-bp chunk edge: IdentifyLocalMEM's chunk grid restarts per sequence, GSAlign.cpp:61-94) and go
 * through all stages together; seed groups never span contigs, AlnBlockVec is kept per contig.  out[k] is EXACTLY what
 * gsa_align_contig(query[k]) returns -- positions, record and string offsets relative to contig k -- and stays valid until the
 * next call on ctx.  n <= 4096, total length < 2^31.  flags: GSA_MANY_DEVICE (query[] are device pointers on ctx's GPU).
 * gsa_align_many bundles contigs of at most 16 Mb by itself (gsa_set_option "bundle_contig"; bundles of about "bundle_cap" = 64 Mb at most). */
int gsa_align_bundle(gsa_ctx *ctx, const char *const *query, const int32_t *qlen, int32_t n, uint32_t flags, gsa_result *out);

/* ---- sequence variants ------------------------------------------------------
 * Replaces VariantIdentification (SeqVariant.cpp:12-119), the step GenomeComparison's caller runs on every finished AlnBlockVec: the
 * walk over the non-seed pairs of all blocks that are not duplicates (:20-29) -- a pure deletion / insertion gives one record
 * (:32-51), a 1 x 1 pair a substitution when the two bases differ and the query's is not ambiguous (:52-63), every other pair is
 * walked column by column over its two gapped strings (:64-115).  The walk runs on the device, on what the alignment left there
 * (records, op strings, the two sequences): nothing but the variants crosses PCIe.
 *
 * one variant, 32 bytes; alleles are pieces of RefSequence / the query, addressed not copied */
typedef struct { int64_t rpos; int32_t qpos, len, chr, pos, kind, block; } gsa_variant;
/* kind: 0 substitution       REF = ref[rpos]            ALT = query[qpos]
         1 insertion record   REF = ref[rpos]            ALT = query[qpos .. qpos+len]     (rpos, qpos = the anchors, i.e. record position - 1)
         2 deletion record    REF = ref[rpos .. rpos+len]  ALT = query[qpos]
         3 insertion in an aligned gap   REF = query[qpos] (sic, SeqVariant.cpp:73-76: the anchor is the first byte of the QUERY piece)   ALT = query[qpos .. qpos+len]
         4 deletion in an aligned gap    REF = ref[rpos .. rpos+len]           ALT = ref[rpos]
   (a .. b inclusive: len + 1 bytes.)  VCF TYPE = {SUBSTITUTE, INSERT, DELETE, INSERT, DELETE}[kind]; len = 0 for kind 0;
   chr = the BLOCK's reference sequence (Variant.chr_idx = ABiter->coor.ChromosomeIdx, :24), pos = GenCoordinateInfo(rpos).gPos, the position's own look-up;
   block = index into gsa_result::blocks.  Order: blocks in result order, records in order, columns in order (the order VarVec grows in). */
typedef struct { int64_t n; const gsa_variant *v; int64_t n_snv, n_ins, n_del; } gsa_variants;
static inline void gsa_variant_alleles(const gsa_variant *v, const char *ref, const char *query,
                                       const char **ref_p, uint32_t *ref_n, const char **alt_p, uint32_t *alt_n)
{
	const char *r = ref + v->rpos, *q = query + v->qpos;
	const uint32_t n = (uint32_t)v->len + 1;
	switch (v->kind) {
	case 1:  *ref_p = r; *ref_n = 1; *alt_p = q; *alt_n = n; break;
	case 2:  *ref_p = r; *ref_n = n; *alt_p = q; *alt_n = 1; break;
	case 3:  *ref_p = q; *ref_n = 1; *alt_p = q; *alt_n = n; break;
	case 4:  *ref_p = r; *ref_n = n; *alt_p = r; *alt_n = 1; break;
	default: *ref_p = r; *ref_n = 1; *alt_p = q; *alt_n = 1; break;
	}
}
/* The variants of the stage-8 result the context holds: valid after gsa_align_contig[_device], gsa_finish_contig, gsa_run_to(8) and
 * gsa_align_bundle, until the next call that changes the context (GSA_ERR_STATE otherwise, and when a prefetch has overwritten the
 * contig's device copy; a contig given as a device buffer must still be there).  k = 0 for a single contig, the contig's index for a
 * bundle: positions and `block` are relative to contig k, i.e. exactly what the single-contig call on query[k] gives; k out of range:
 * GSA_ERR_ARG.  No blocks: n = 0.  Memory is owned by the context and valid until the next call on it. */
int gsa_call_variants(gsa_ctx *ctx, int32_t k, gsa_variants *out);
/* measurement: device time (two hipEvents around the pass on the library's stream) of the gsa_call_variants passes of this context since
 * gsa_set_profiling(ctx, 8) switched that timing on, and their number; without that flag nothing is recorded and both stay 0 */
int gsa_get_variant_timing(gsa_ctx *ctx, double *ms_sum, int64_t *n_calls);
/* gsa_align_many with the variant pass run by the worker in front of the callback: *var is valid during the callback only, like *res */
typedef int (*gsa_result_var_fn)(void *user, int32_t contig, const gsa_result *res, const gsa_variants *var);
int gsa_align_many_variants(gsa_ctx *const *ctx, int32_t n_ctx, const char *const *query, const int32_t *qlen, int32_t n,
                            uint32_t flags, gsa_result_var_fn on_result, void *user);

/* ---- per-block CIGARs (PAF's cg:Z:) -------------------------------------------
 * The CIGAR of a block is the run-length encoding of the columns of the two `s` lines OutputMAF prints for it (tools.cpp:165-216), in the
 * order they are printed: for a reverse-strand block after SelfComplementarySeq, i.e. in reference-forward order.  The reference row is
 * PAF's target, the query row PAF's query.  Column classes (BAM op codes):
 *   I (1)  the reference row holds '-'                D (2)  the query row holds '-'
 *   = (7)  both rows hold a base and the two are the same one of A/C/G/T, whatever their case
 *   X (8)  both rows hold a base, in every other case -- N and IUPAC codes on either side included
 * A seed record is `len` columns of '=' (an exact match over A/C/G/T; OutputMAF prints the query text on both lines for it).  Adjacent runs
 * of one class merge ACROSS record boundaries: two seeds with nothing between them are one '=' run.  An op is len << 4 | code (len < 2^28).
 * This is NOT the reference's score rule: CountIdenticalPairs counts N against N (and N against '-') as identical and
 * CheckFragPairMismatch forgives every ambiguous query base, so the '=' columns of a block may differ from gsa_block::score where
 * ambiguous bases sit in gaps.
 * The walk runs on the device, over what the alignment left there (records, op strings, the two sequences).  It describes the result as
 * gsa_result holds it, UNTRIMMED: the iExtension trim of a block that runs past the end of its reference sequence (tools.cpp:192-202)
 * is the emitter's business, as it is for MAF text. */
typedef struct { int64_t cig_off; int32_t n_cig; int32_t n_eq, n_x, n_ins, n_del; int32_t _pad; } gsa_block_cigar;  /* columns per class; one entry per block of gsa_result::blocks, same order */
typedef struct { int32_t n_blocks; int64_t n_ops; const gsa_block_cigar *blk; const uint32_t *ops; } gsa_cigars;
#define GSA_CIGAR_INS 1u
#define GSA_CIGAR_DEL 2u
#define GSA_CIGAR_EQ  7u
#define GSA_CIGAR_X   8u
/* n ops as PAF's cg string (decimal length, then the op letter) into buf[cap], NUL-terminated.  Returns the length of the whole string
 * without the NUL -- at most 10 bytes per op; when that is >= cap the string was cut and buf holds its first cap - 1 bytes. */
static inline size_t gsa_cigar_string(const uint32_t *ops, int64_t n, char *buf, size_t cap)
{
	static const char letter[16] = { 'M', 'I', 'D', 'N', 'S', 'H', 'P', '=', 'X', '?', '?', '?', '?', '?', '?', '?' };
	size_t at = 0;
	for (int64_t i = 0; i < n; i++) {
		char tmp[12]; int m = 0; uint32_t len = ops[i] >> 4;
		do { tmp[m++] = (char)('0' + len % 10); len /= 10; } while (len);
		while (m) { --m; if (at + 1 < cap) buf[at] = tmp[m]; at++; }
		if (at + 1 < cap) buf[at] = letter[ops[i] & 15u];
		at++;
	}
	if (cap) buf[at < cap ? at : cap - 1] = '\0';
	return at;
}
/* The CIGARs of ALL blocks of the stage-8 result the context holds, duplicates included (the caller filters).  Validity and call order are
 * those of gsa_call_variants: after gsa_align_contig[_device], gsa_finish_contig, gsa_run_to(8) and gsa_align_bundle, until the next call
 * that changes the context (GSA_ERR_STATE otherwise, and when a prefetch has overwritten the contig's device copy).  k = 0 for a single
 * contig, the contig's index for a bundle; k out of range: GSA_ERR_ARG.  No blocks: n_blocks = 0.  blk[b].cig_off indexes `ops`.
 * Memory is owned by the context and valid until the next call on it. */
int gsa_block_cigars(gsa_ctx *ctx, int32_t k, gsa_cigars *out);
/* measurement: host wall time the calling threads spent inside gsa_block_cigars on this context since it was created (launches, the two waits,
 * the copies home), and the number of calls.  Always on (two clock reads per call). */
int gsa_get_cigar_timing(gsa_ctx *ctx, double *ms_sum, int64_t *n_calls);
/* ---- per-block cs strings (PAF's cs:Z:, short form) ---------------------------
 * The cs of a block is a function of the block's CIGAR ops, in the order gsa_block_cigars delivers them (output order, i.e. reference-forward:
 * a reverse-strand block's ops are stored reversed), and of the bases under them.  Each op gives one token group:
 *   = run of n columns   ':' and decimal n
 *   X run of n columns   n groups "*rq": r the reference letter, q the query letter of that column
 *   I run of n columns   '+' and the n query letters
 *   D run of n columns   '-' and the n reference letters
 * The letter of a byte b is "acgtn"[nt4(b)] in a forward-strand block (bdir != 0) and "tgcan"[nt4(b)] in a reverse-strand block, whose columns are
 * taken back to front; nt4 maps A/C/G/T in either case to 0..3 and everything else to 4.  For a reverse-strand block the byte comes from the
 * reverse-complement half of the 2G text and from the query as stored, so the letters printed are the forward-strand reference base and the
 * complemented query base: what the two `s` lines of OutputMAF show after SelfComplementarySeq, lower-cased, with every byte outside acgt
 * printed as 'n' (the reference's ReverseMap turns IUPAC codes into NUL there; 'n' is the defined answer here).  The classes are the CIGAR's:
 * N against N is an X column and prints "*nn", a difference in case only is '='.  Only the short form exists (the long form, "=ACGT...", is as
 * large as the genome).  Like the CIGAR the answer is UNTRIMMED: the iExtension trim is the emitter's business.
 * blk[b] = where block b's string lies in `cs` and its length; the strings are not NUL-terminated. */
typedef struct { int64_t cs_off; int32_t n_cs; int32_t _pad; } gsa_cs_block;                           /* 16 bytes; one per block of gsa_result::blocks, same order */
typedef struct { int32_t n_blocks; int64_t n_bytes; const gsa_cs_block *blk; const char *cs; } gsa_cs; /* 32 bytes */
/* The cs strings of ALL blocks of the stage-8 result the context holds, duplicates included.  Validity, call order, k and the error codes are
 * those of gsa_block_cigars (GSA_ERR_STATE before stage 8 and after a prefetch has overwritten the contig, GSA_ERR_ARG for k out of range; no
 * blocks: n_blocks = 0, n_bytes = 0).  The call runs the CIGAR pass itself; a later gsa_block_cigars or gsa_call_variants on the same result
 * returns what it returned before -- the three answers live in buffers of their own.  A block whose string reaches 2^31 bytes: GSA_ERR_LIMIT.
 * Memory is owned by the context and valid until the next call on it; the bytes come home in one copy into pinned memory. */
int gsa_block_cs(gsa_ctx *ctx, int32_t k, gsa_cs *out);
/* measurement: host wall time the calling threads spent inside gsa_block_cs on this context since it was created (its CIGAR pass included), and
 * the number of calls.  Always on. */
int gsa_get_cs_timing(gsa_ctx *ctx, double *ms_sum, int64_t *n_calls);

/* ---- lifting reference positions through the alignment ------------------------
 * Where does a position of the reference lie on the query contig?  A reference position is a 0-based FORWARD global coordinate p in [0, G): the offset in
 * the concatenation of the reference sequences.  It is text position p for forward-strand blocks and 2G - 1 - p for reverse-strand blocks (the mapping
 * of GenCoordinateInfo, tools.cpp:120-140).
 *   coverage  a block covers text position t when first.rpos <= t < end, end = last.rpos + last.rlen CLAMPED to the end of the block's chromosome copy: unlike the
 *             CIGAR and cs answers this one is TRIMMED (the iExtension rule, tools.cpp:192-202) -- an untrimmed overrun would claim positions of the neighbouring sequence
 *   choice    among the blocks that cover either text position of p: bdup == 0 before bdup != 0, then the greater gsa_block::score, then the smaller block index;
 *             n_cover counts ALL covering blocks, duplicates included, and saturates at 65535
 *   class     of the chosen block's column that holds the reference base, with the CIGAR's codes and the CIGAR's rule:
 *             GSA_CIGAR_EQ / GSA_CIGAR_X  the base faces a query base: qpos = that base's 0-based position in the contig as stored (forward, whatever the strand)
 *             GSA_CIGAR_DEL               the base faces '-': qpos = the query base consumed last in front of the column in walk order (it always exists: a gap follows a seed)
 * The columns are the ones the CIGAR pass reads: a seed record is '=' over its whole length, an equal-length gap that needed no DP is classified by comparing the
 * two bases, a DP gap is read from the op string of its DP job.  One hit per position that some block covers, ascending in idx; positions no block covers are absent. */
typedef struct { int32_t idx;      /* index into the positions given to gsa_lift_set */
                 int32_t qpos; int32_t block;   /* block: index among contig k's blocks (gsa_result::blocks) */
                 uint8_t cls, rev; uint16_t n_cover; } gsa_lift_hit;          /* 16 bytes; rev = 1: the chosen block lies on the reverse strand */
typedef struct { int64_t n_hits; const gsa_lift_hit *hits; } gsa_lifts;
/* The positions to lift: n of them are copied to the context's device and stay until the next gsa_lift_set or gsa_destroy; n = 0 clears them.  A clone starts
 * without positions.  A position outside [0, G): GSA_ERR_ARG with the first offender in gsa_last_error, nothing changed.  n >= 2^31 - 256: GSA_ERR_LIMIT.
 * Device memory: about 8 (the position) + 16 (its hit) + 8 (its chosen block and n_cover between the two launches) bytes per position. */
int gsa_lift_set(gsa_ctx *ctx, const int64_t *pos, int64_t n);
/* The positions of gsa_lift_set lifted through the stage-8 result the context holds.  Validity, call order, k and the error codes are those of gsa_block_cigars;
 * without positions GSA_ERR_STATE.  No blocks or no hits: n_hits = 0.  In a bundle qpos is relative to contig k, i.e. what the single-contig call on query[k]
 * gives.  The answer lives in buffers of its own: a later gsa_block_cigars, gsa_block_cs or gsa_call_variants returns what it returned before, and so does
 * this call after one of them.  Memory is owned by the context and valid until the next call on it; the hits come home in one copy into pinned memory. */
int gsa_lift(gsa_ctx *ctx, int32_t k, gsa_lifts *out);
/* measurement: host wall time the calling threads spent inside gsa_lift on this context since it was created, and the number of calls.  Always on. */
int gsa_get_lift_timing(gsa_ctx *ctx, double *ms_sum, int64_t *n_calls);

/* ---- per-window reference track ----------------------------------------------------
 * How much of each reference sequence is aligned, how diverged, and where are the holes?  The reference sequences are cut into windows of W bases; the grid restarts at
 * every sequence: sequence c of length L has ceil(L / W) windows, window j covers the local positions [j W, min((j + 1) W, L)), no window spans two sequences.
 *   blocks    only the blocks of contig k with bdup == 0 are counted (the set gsa_call_variants walks)
 *   coverage  TRIMMED exactly as gsa_lift trims it: a block covers the text positions first.rpos <= t < end, end = last.rpos + last.rlen clamped to the end of the block's
 *             chromosome copy; text position t is forward position t for a forward-strand block and 2G - 1 - t for a reverse-strand block.  (The per-base clamp, not the
 *             reference's cut of iExtension COLUMNS: the two agree wherever the overrun lies inside a final seed.)
 *   columns   the CIGAR's classes by the CIGAR's rule: a seed record is '=' over its length, an equal-length gap that needed no DP is classified base against base, a DP
 *             gap is read from the op string of its DP job, a pure deletion / insertion record is one class throughout
 *   n_cov     bases of the window covered by at least one counted block (the union: n_cov <= len)
 *   n_eq, n_x, n_del   columns of that class whose reference base lies in the window and is covered (t < end), summed over ALL counted blocks: a base under two blocks
 *             counts twice, n_eq + n_x + n_del is the depth sum
 *   n_ins     inserted query bases (CIGAR I columns), summed over all counted blocks; each belongs to the reference base consumed last in front of it in WALK order (it
 *             exists: a gap follows a seed) and is dropped exactly when that base is trimmed
 * One record per window with n_cov > 0, ascending by (chr, start). */
typedef struct { int32_t chr, start, len; uint32_t n_cov, n_eq, n_x, n_del, n_ins; } gsa_track_win;   /* 32 bytes; start 0-based inside the sequence */
typedef struct { int64_t n_win; const gsa_track_win *win; } gsa_tracks;
/* The window length W of this context from now on; 0 clears it.  A clone starts without a window.  W < 0: GSA_ERR_ARG.  A total of 2^31 - 256 windows or more over all
 * reference sequences: GSA_ERR_LIMIT, nothing changed.  Device memory: 16 bytes per window of the reference (allocated and cleared by the first gsa_ref_track after the
 * call, kept clear by the pass itself) + 32 per window that comes home. */
int gsa_track_set(gsa_ctx *ctx, int32_t window);
/* The track of the stage-8 result the context holds.  Validity, call order, k and the error codes are those of gsa_block_cigars; without a window GSA_ERR_STATE.  No counted
 * block: n_win = 0.  The counts are uint32_t: when the reference bases plus the query bases that the counted blocks of contig k span (last record's end minus first record's
 * start on either side, summed over the blocks -- no count can exceed the sum of the columns, which this bounds) exceed 2^32 - 1, GSA_ERR_LIMIT before any launch.  The answer
 * lives in buffers of its own: the eight other passes return what they returned before, and so does this call after one of them.  Memory is owned by the context and valid
 * until the next call on it; the windows come home in one copy into pinned memory. */
int gsa_ref_track(gsa_ctx *ctx, int32_t k, gsa_tracks *out);
/* measurement: host wall time the calling threads spent inside gsa_ref_track on this context since it was created, and the number of calls.  Always on. */
int gsa_get_track_timing(gsa_ctx *ctx, double *ms_sum, int64_t *n_calls);

/* ---- per-window query track ----------------------------------------------------------
 * The mirror image of the reference track: which parts of the QUERY contig align at all, how diverged are they, where are the holes, and which stretches align to two
 * places at once?  Query contig k of qlen bases is cut into ceil(qlen / W) windows, window j covers [j W, min((j + 1) W, qlen)).  Positions are 0-based in the contig as
 * stored, whatever the strand of a block (records hold contig positions as stored; the reference is the side that is reverse-complemented); in a bundle they are
 * relative to contig k, as gsa_lift's qpos is.
 *   blocks    only the blocks of contig k with bdup == 0 and a valid chr are counted: gsa_ref_track's set
 *   columns   the CIGAR pass's classes by its rule: a seed is '=' over its length, an equal-length gap that needed no DP is classified base against base, a DP gap is
 *             read from the op string of its DP job, a pure insertion / deletion record is one class throughout
 *   kept      TRIMMED exactly as gsa_ref_track trims: end = last.rpos + last.rlen clamped to the end of the block's chromosome copy; an '=', 'X' or 'D' column is kept
 *             when its reference text position is t < end, an 'I' column when the reference base consumed last in front of it in walk order is kept.  t ascends in walk
 *             order, so the kept columns are a PREFIX of the block's columns, and the query bases of the kept '=' / 'X' / 'I' columns are one interval [q0, q1) per block
 *   n_cov     bases of the window under at least one counted block's [q0, q1) (the union: n_cov <= len)
 *   n_multi   bases of the window under at least two (n_multi <= n_cov)
 *   n_eq, n_x, n_ins   kept columns of that class whose query base lies in the window, summed over ALL counted blocks: a base under two blocks counts twice,
 *             n_eq + n_x + n_ins is the depth sum (>= n_cov, equal exactly where n_multi == 0)
 *   n_del     kept 'D' columns (reference bases facing '-'), each charged to the query base consumed last in front of it in walk order (it exists: a gap follows a seed)
 * One record per window with n_cov > 0, ascending by start. */
typedef struct { int32_t start, len; uint32_t n_cov, n_multi, n_eq, n_x, n_ins, n_del; } gsa_qtrack_win;   /* 32 bytes; start 0-based inside the contig */
typedef struct { int64_t n_win; const gsa_qtrack_win *win; } gsa_qtracks;
/* The query-side window length W of this context from now on; 0 clears it.  A clone starts without a window.  W < 0: GSA_ERR_ARG.  Independent of gsa_track_set: both
 * windows may be set, with different lengths.  Device memory: 16 bytes per window of the longest contig seen (allocated and cleared by the gsa_query_track that first
 * needs them, kept clear by the pass itself) + 32 per window that comes home. */
int gsa_qtrack_set(gsa_ctx *ctx, int32_t window);
/* The query track of the stage-8 result the context holds.  Validity, call order, k and the error codes are those of gsa_block_cigars; without a window GSA_ERR_STATE.  No
 * counted block: n_win = 0.  The counts are uint32_t, with gsa_ref_track's rule: when the reference bases plus the query bases that the counted blocks of contig k span
 * exceed 2^32 - 1, GSA_ERR_LIMIT before any launch.  A DP record without a job, or a column outside its record or sequence, is counted on the device and fails the call
 * with GSA_ERR_STATE.  The answer lives in buffers of its own: the eight other passes return what they returned before, in any call order, and so does this call after
 * one of them.  Memory is owned by the context and valid until the next call on it; the windows come home in one copy into pinned memory. */
int gsa_query_track(gsa_ctx *ctx, int32_t k, gsa_qtracks *out);
/* measurement: host wall time the calling threads spent inside gsa_query_track on this context since it was created, and the number of calls.  Always on. */
int gsa_get_qtrack_timing(gsa_ctx *ctx, double *ms_sum, int64_t *n_calls);

/* ---- per-block chain segments (UCSC chain files, for liftOver / CrossMap / bcftools +liftover) --------------
 * ("Chain" already names the seed-chaining stage of this library: the word for the new thing is SEGS.)
 * For every block of gsa_result::blocks take its columns in OUTPUT order -- the order in which gsa_block_cigars delivers ops: reference-forward, so a
 * reverse-strand block is taken back to front.
 *   aligned column   CIGAR class '=' or 'X'
 *   gap column       class 'I' or 'D'
 *   segment          a maximal run of aligned columns
 *   gap              the gap columns between two segments: dt counts its D columns (reference bases facing '-'), dq its I columns (query bases facing '-').
 *                    Both may be non-zero (an I run that touches a D run), never both zero.
 * A block with n segments gives n triples {size, dt, dq}, the gap being the one BEHIND the segment in output order; the last triple has dt = dq = 0.  These
 * are the data lines of a chain.  Like the CIGAR and cs answers this one is UNTRIMMED: the iExtension trim is the emitter's business (gsah_segs_trim in
 * libgsa_host.so cuts triples).  An untrimmed block starts and ends with a seed, so with a segment; a block without records gives no segment.
 * blk[b] = where block b's triples lie in `seg` and how many there are. */
typedef struct { int32_t size, dt, dq; } gsa_seg;                                  /* 12 bytes */
typedef struct { int64_t seg_off; int32_t n_seg; int32_t _pad; } gsa_seg_block;   /* 16 bytes; one per block of gsa_result::blocks, same order */
typedef struct { int32_t n_blocks; int64_t n_segs; const gsa_seg_block *blk; const gsa_seg *seg; } gsa_segs;   /* 32 bytes */
/* The triples of ALL blocks of the stage-8 result the context holds, duplicates included (the caller filters).  Validity, call order, k and the error codes are
 * those of gsa_block_cigars: before stage 8, or after a prefetch has overwritten the contig, GSA_ERR_STATE; k out of range GSA_ERR_ARG; no blocks: n_blocks = 0.
 * The call runs the CIGAR walk itself (its errors pass through) and then four launches at run granularity -- no column is looked at twice.  2^31 - 256 segments
 * or more: GSA_ERR_LIMIT.  The answer lives in buffers of its own: gsa_block_cigars, gsa_block_cs, gsa_call_variants, gsa_lift and gsa_ref_track return what
 * they returned before, and so does this call after one of them.  Memory is owned by the context and valid until the next call on it; block table and triples
 * come home in one copy each into pinned memory.  Device memory: 4 bytes per CIGAR op + 32 per segment. */
int gsa_block_segs(gsa_ctx *ctx, int32_t k, gsa_segs *out);
/* measurement: host wall time the calling threads spent inside gsa_block_segs on this context since it was created (its CIGAR pass included), and the
 * number of calls.  Always on. */
int gsa_get_seg_timing(gsa_ctx *ctx, double *ms_sum, int64_t *n_calls);

/* ---- the query projected onto the reference ------------------------------------------------------------------
 * One character per forward reference position p in [0, G): the query base the best alignment puts there, '-' where the base is deleted, a marker where nothing
 * aligns -- accumulated over every contig (context, device) that paints.  The only pass whose answer is not per contig.
 *   accumulator  one uint32_t word per p; 0: uncovered, else
 *                  bit 31      bdup == 0 of the painting block
 *                  bits 30..3  min(max(gsa_block::score, 0), 2^28 - 1)
 *                  bits 2..0   code: 1 A, 2 C, 3 G, 4 T, 5 N, 6 gap
 *   painting     a block's covered text positions are first.rpos <= t < end, end = last.rpos + last.rlen CLAMPED to the end of the block's chromosome copy -- TRIMMED
 *                exactly as gsa_lift trims; p = t for a forward-strand block, 2G - 1 - t for a reverse-strand block.  The columns are the CIGAR pass's: a seed is '='
 *                over its length, an equal-length gap that needed no DP faces base to base, a DP gap is read from the op string of its DP job, a pure deletion is gap
 *                throughout; inserted query bases have no reference base and are not projected.  A reference base that faces a query byte gets that byte's code --
 *                acgtACGT 1..4, anything else 5 -- complemented on a reverse-strand block (5 - code for 1..4, 5 stays): the character the MAF prints in the query row
 *                of that column.  A reference base that faces '-' gets code 6.  Every covered column offers key | code to word p and the word keeps the MAXIMUM.
 *   order        so: a block that is no duplicate before a duplicate, then the greater (clamped) score, then the greater code.  gsa_lift breaks score ties by the
 *                smaller block index; here the tie rule is chosen so that the result does not depend on the order in which blocks, contigs, contexts and devices
 *                arrive.  Wherever the two best covering blocks differ in (dup, clamped score) the character is the one gsa_lift's hit implies: query[qpos]
 *                (complemented when rev) for '=' / 'X', '-' for 'D'.
 *   text         codes 1..6 -> A C G T N -, word 0 -> n. */
#define GSA_PROJ_NO_DUP 1u   /* blocks with bdup != 0 are not painted (the CLI's -unique) */
typedef struct { int32_t n_blocks; int32_t _pad; int64_t n_cols; } gsa_proj_stat;   /* 16 bytes: blocks painted, words offered */
/* An accumulator for the context.  share == NULL: G zeroed words on the context's device (4 bytes per reference base: 12.4 GB for a human reference); a failed
 * allocation is GSA_ERR_NOMEM with nothing changed.  share != NULL: that context's accumulator, which must lie on the SAME device (else GSA_ERR_ARG, the reason
 * in gsa_last_error) -- both contexts then paint into the one array (integer maxima from several streams commute).  The array is reference counted:
 * gsa_proj_close and gsa_destroy drop a reference, the last one frees it once the stream is quiet.  A clone starts without an accumulator.  A context that
 * holds one already: GSA_ERR_STATE; unknown flags: GSA_ERR_ARG. */
int gsa_proj_open(gsa_ctx *ctx, gsa_ctx *share, uint32_t flags);
int gsa_proj_close(gsa_ctx *ctx);   /* without an accumulator: GSA_ERR_STATE */
int gsa_proj_clear(gsa_ctx *ctx);   /* every word back to 0 (and the array no longer dirty, see gsa_project) */
/* Paints the blocks of the stage-8 result the context holds (contig k of a bundle: the painted content does not depend on whether the contig was aligned alone or in
 * a bundle).  Validity, call order, k and the error codes are those of gsa_block_cigars; without an accumulator GSA_ERR_STATE.  No blocks: the stat is zero, the
 * words untouched.  The pass has buffers of its own: the eight other passes return what they returned before, in any call order.  A DP record without a job, or a
 * column outside its record or sequence, is counted on the device and fails the call with GSA_ERR_STATE; the accumulator is then DIRTY, and gsa_proj_fetch and
 * gsa_project return GSA_ERR_STATE on it until gsa_proj_clear.  out may be NULL. */
int gsa_project(gsa_ctx *ctx, int32_t k, gsa_proj_stat *out);
/* Positions [p0, p0 + n) as characters (text, n bytes, no NUL) and / or as words; either may be NULL.  A range outside [0, G) or n < 0: GSA_ERR_ARG; n == 0: nothing
 * happens.  Fetch and merge wait for the context's OWN stream only: the caller orders them against other contexts that share the array (gsa_align_many_ex has
 * returned by then).  The characters are made on the device; everything comes home through pinned staging in bounded chunks. */
int gsa_proj_fetch(gsa_ctx *ctx, int64_t p0, int64_t n, char *text, uint32_t *words);
/* Host words (another device's, another run's) into positions [p0, p0 + n): uploaded in bounded chunks, the element-wise maximum stays. */
int gsa_proj_merge(gsa_ctx *ctx, int64_t p0, int64_t n, const uint32_t *words);
/* measurement: host wall time the calling threads spent inside gsa_project on this context since it was created, and the number of calls.  Always on. */
int gsa_get_proj_timing(gsa_ctx *ctx, double *ms_sum, int64_t *n_calls);

/* ---- lifting reference intervals through the alignment ------------------------------------------------------
 * Where does an annotated interval of the reference (a gene, an exon, a BED line) lie on the query contig, and how well is it conserved?  A REGION is a half-open
 * interval [beg, end) of 0-based FORWARD global reference coordinates, 0 <= beg < end <= G, inside ONE reference sequence.  It is the text interval [beg, end) for
 * forward-strand blocks and [2G - end, 2G - beg) for reverse-strand blocks (t = p and t = 2G - 1 - p, as for gsa_lift).
 *   coverage  gsa_lift's, TRIMMED: a block covers the text positions first.rpos <= t < min(last.rpos + last.rlen, end of the block's chromosome copy)
 *   choice    among the blocks of contig k whose coverage overlaps the region in either orientation: bdup == 0 before bdup != 0, then the greater OVERLAP (the region
 *             bases under the block's coverage), then the greater gsa_block::score, then the smaller block index.  gsa_lift has no overlap to compare; for a region
 *             of length 1 every overlap is 1 and the choice is exactly gsa_lift's.  n_cover counts ALL overlapping blocks, duplicates included, and saturates at 65535
 *   span      [t_lo, t_hi): the part of the region's text interval under the chosen block's coverage -- one interval.  The answer is about the block's columns in WALK
 *             order from the column that holds reference base t_lo through the column that holds t_hi - 1, both included
 *   classes   the CIGAR pass's, by its rule: a seed is '=' throughout, an equal-length gap that needed no DP is classified base against base, a DP gap is read from the
 *             op string of its DP job, a pure deletion or insertion record is one class throughout
 *   n_eq, n_x, n_del   columns of that class in the span; each holds a reference base of the span: n_eq + n_x + n_del == t_hi - t_lo
 *   n_ins     the I columns strictly inside the span; inserted bases in front of its first or behind its last reference-bearing column are not counted
 *   q_lo      the first query base at or behind the span's first column in walk order, 0-based in the contig as stored, whatever the strand: gsa_lift's qpos of t_lo
 *             when that column is '=' / 'X', qpos + 1 when it is 'D'
 *   q_hi      q_lo + n_eq + n_x + n_ins; a span wholly inside a deletion has q_lo == q_hi.  In a bundle q_lo and q_hi are relative to contig k
 * The counts cannot overflow: a span is shorter than its reference sequence and its query bases are fewer than the contig's, both < 2^31.
 * One hit per region that some block overlaps, ascending in idx; regions no block overlaps are absent. */
typedef struct { int32_t idx, block;          /* index into the regions given to gsa_regions_set; block among contig k's blocks (gsa_result::blocks) */
                 int32_t off_lo, off_hi;      /* the covered part of the region in FORWARD coordinates, relative to beg: [beg + off_lo, beg + off_hi) */
                 int32_t q_lo, q_hi;
                 uint32_t n_eq, n_x, n_del, n_ins;
                 uint8_t rev, _pad0; uint16_t n_cover; int32_t _pad1; } gsa_region_hit;   /* 48 bytes; rev = 1: the chosen block lies on the reverse strand */
typedef struct { int64_t n_hits; const gsa_region_hit *hits; } gsa_region_lifts;
/* The regions to lift: n of them are copied to the context's device and stay until the next gsa_regions_set or gsa_destroy; n = 0 clears them.  A clone starts
 * without regions.  A region outside [0, G), empty, reversed or crossing a sequence boundary: GSA_ERR_ARG with the first offender and its entry number in
 * gsa_last_error, nothing changed.  n >= 2^31 - 256: GSA_ERR_LIMIT.  Device memory: about 16 (the region) + 48 (its hit) + 8 (its chosen block and n_cover
 * between the launches) bytes per region, and 16 bytes per record of the result for the class prefix. */
int gsa_regions_set(gsa_ctx *ctx, const int64_t *beg, const int64_t *end, int64_t n);
/* The regions of gsa_regions_set lifted through the stage-8 result the context holds.  Validity, call order, k and the error codes are those of gsa_block_cigars;
 * without regions GSA_ERR_STATE.  No blocks or no hits: n_hits = 0.  A DP record without a job, or a span the records do not reach, is counted on the device and
 * fails the call with GSA_ERR_STATE.  The answer lives in buffers of its own: the eight other passes return what they returned before, in any call order, and so
 * does this call after one of them.  Memory is owned by the context and valid until the next call on it; the hits come home in one copy into pinned memory. */
int gsa_lift_regions(gsa_ctx *ctx, int32_t k, gsa_region_lifts *out);
/* measurement: host wall time the calling threads spent inside gsa_lift_regions on this context since it was created, and the number of calls.  Always on. */
int gsa_get_region_timing(gsa_ctx *ctx, double *ms_sum, int64_t *n_calls);

/* gsa_align_many with optional passes run by the worker in front of the callback -- before the prefetch after next can touch the contig's
 * slot: `want` = GSA_WANT_VARIANTS (gsa_call_variants) | GSA_WANT_CIGARS (gsa_block_cigars) | GSA_WANT_CS (gsa_block_cs) | GSA_WANT_LIFT (gsa_lift) | GSA_WANT_TRACK (gsa_ref_track) | GSA_WANT_SEGS (gsa_block_segs) | GSA_WANT_PROJ (gsa_project) | GSA_WANT_REGIONS (gsa_lift_regions) | GSA_WANT_QTRACK (gsa_query_track).  *ex and what it
 * points to are valid during the callback only, like *res. */
#define GSA_WANT_VARIANTS 1u
#define GSA_WANT_CIGARS   2u
#define GSA_WANT_CS       4u   /* gsa_block_cs; implies GSA_WANT_CIGARS */
#define GSA_WANT_LIFT     16u  /* gsa_lift of every contig; every context of ctx[] must hold positions (gsa_lift_set), else GSA_ERR_STATE before any contig is aligned */
#define GSA_WANT_TRACK    32u  /* gsa_ref_track of every contig; every context of ctx[] must hold a window (gsa_track_set), else GSA_ERR_STATE before any contig is aligned */
#define GSA_WANT_SEGS     64u  /* gsa_block_segs; implies GSA_WANT_CIGARS */
#define GSA_WANT_PROJ     128u /* gsa_project of every contig, behind the other passes; it adds nothing behind gsa_extras; every context of ctx[] must hold an accumulator (gsa_proj_open), else GSA_ERR_STATE before any contig is aligned -- but where NO context of ctx[] holds one the bit is refused like an unknown one, GSA_ERR_ARG, as it was before the pass existed */
#define GSA_WANT_REGIONS  256u /* gsa_lift_regions of every contig; every context of ctx[] must hold regions (gsa_regions_set), else GSA_ERR_STATE before any contig is aligned */
#define GSA_WANT_QTRACK   512u /* gsa_query_track of every contig; every context of ctx[] must hold a query-side window (gsa_qtrack_set), else GSA_ERR_STATE before any contig is aligned */
typedef struct { const gsa_variants *var; const gsa_cigars *cig; } gsa_extras;   /* NULL where not asked for */
/* The contig's cs strings inside the callback of gsa_align_many_ex: the library hands the callback a LARGER object whose head is the gsa_extras
 * (which keeps its two members and its 16 bytes), and this call reaches what lies behind it -- so it is valid for the `ex` the library passed
 * only, never for a gsa_extras the caller made.  GSA_ERR_STATE when GSA_WANT_CS was not asked for.  *out is valid during the callback only. */
int gsa_extras_cs(const gsa_extras *ex, gsa_cs *out);
/* The contig's lifted positions inside the callback, in the same way (GSA_ERR_STATE when GSA_WANT_LIFT was not asked for). */
int gsa_extras_lift(const gsa_extras *ex, gsa_lifts *out);
/* The contig's track inside the callback, in the same way (GSA_ERR_STATE when GSA_WANT_TRACK was not asked for). */
int gsa_extras_track(const gsa_extras *ex, gsa_tracks *out);
/* The contig's chain segments inside the callback, in the same way (GSA_ERR_STATE when GSA_WANT_SEGS was not asked for). */
int gsa_extras_segs(const gsa_extras *ex, gsa_segs *out);
/* The contig's lifted regions inside the callback, in the same way (GSA_ERR_STATE when GSA_WANT_REGIONS was not asked for). */
int gsa_extras_regions(const gsa_extras *ex, gsa_region_lifts *out);
/* The contig's query track inside the callback, in the same way (GSA_ERR_STATE when GSA_WANT_QTRACK was not asked for). */
int gsa_extras_qtrack(const gsa_extras *ex, gsa_qtracks *out);
typedef int (*gsa_result_ex_fn)(void *user, int32_t contig, const gsa_result *res, const gsa_extras *ex);
int gsa_align_many_ex(gsa_ctx *const *ctx, int32_t n_ctx, const char *const *query, const int32_t *qlen, int32_t n,
                      uint32_t flags, uint32_t want, gsa_result_ex_fn on_result, void *user);

/* ---- the index itself ---------------------------------------------------------
 * sizes of the two arrays gsa_build_index fills, for a forward length G: pure arithmetic, no device */
int gsa_index_sizes(int64_t G, uint64_t *bwt_words, uint64_t *n_sa);
/* Replaces bwa_idx_build's BWT/SA half (BWT_Index/bwtindex.c:77-149, bwt.c:101-123): pac = the .pac bytes of G bases (bntseq.c:192-201;
 * only the first ceil(G/4) are read) -> primary, L2[5], the interleaved bwt words and the sampled SA exactly as the .bwt / .sa files and
 * gsa_index_view hold them.  Host pointers out.  No context needed; thread-safe per device.
 * The text the suffixes of which are sorted is forward + reverse complement + '$' (2G + 1 suffixes); the device sorts them by prefix doubling on 32-bit
 * suffix indices, so G <= 1 073 741 822 (GSA_ERR_LIMIT above that, before anything is allocated; ~52 bytes of device memory per suffix, GSA_ERR_NOMEM when
 * they are not there).  Errors in this order: NULL pointers or G <= 0 GSA_ERR_ARG, G over the bound GSA_ERR_LIMIT, no device GSA_ERR_HIP;
 * gsa_last_error(NULL) has the text. */
int gsa_build_index(int device, const uint8_t *pac, int64_t G, uint64_t *primary, uint64_t L2[5], uint32_t *bwt, uint64_t *sa);
/* measurement: device ms and doubling rounds of the last gsa_build_index / gsa_build_index_opts of the calling thread */
int gsa_get_index_build_stats(double *ms, int32_t *rounds);
/* gsa_build_index with a choice of sorter.  flags: GSA_BUILD_AUTO -- the sorter of gsa_build_index up to its bound of 1 073 741 822 bases, the wide one above it;
 * GSA_BUILD_WIDE -- the wide one at any size.  The wide sorter keeps suffix numbers, ranks and SA slots in 64 bits and works in BATCHES: ranges of classes of
 * the first 8 bases that hold at most batch_cap suffixes each (0: 2^30; a class larger than the cap is a batch of its own, and a class of more than
 * 2 147 483 646 suffixes GSA_ERR_LIMIT with the class in the message), sorted one after the other with the 32-bit radix sort.  The running symbol counts of
 * the .bwt layout are scanned in segments of occ_segment 128-symbol blocks (0, or more than 2^23: 2^23) with a 64-bit carry.  The arrays are the same bytes
 * whichever sorter made them.  Device memory: 16 bytes per suffix, 52 per suffix of the largest batch, 24 per suffix that still ties with another after 29
 * bases (GSA_ERR_NOMEM, with the sizes, when that list does not fit).
 * The bound: G <= 4 294 967 295 -- a sort key holds a rank inside a batch (31 bits) and a rank in the text (33 bits); the file layout and gsa_index_sizes (64-bit
 * counts and samples) would allow more.  Errors in this order: NULL pointers or G <= 0, an unknown flag, a negative batch_cap or occ_segment GSA_ERR_ARG;
 * G over the bound GSA_ERR_LIMIT; no device GSA_ERR_HIP. */
#define GSA_BUILD_AUTO 0u
#define GSA_BUILD_WIDE 1u
int gsa_build_index_opts(int device, const uint8_t *pac, int64_t G, uint32_t flags, int64_t batch_cap, int64_t occ_segment,
                         uint64_t *primary, uint64_t L2[5], uint32_t *bwt, uint64_t *sa);
/* measurement, beside gsa_get_index_build_stats: the batches that held a suffix (0: the narrow sorter ran), the peak of device memory in use during the last
 * gsa_build_index_opts of the calling thread (the low-water mark of hipMemGetInfo below its value at the start; the list of tied suffixes is given the free
 * memory up to 24 bytes per suffix, so this says that the build fits, not what it needs) and the suffixes that still tied with another after the first pass (29
 * bases): the longest that list ever is.  0, 0, 0 for the narrow sorter. */
int gsa_get_index_build_stats2(int64_t *batches, uint64_t *peak_bytes, int64_t *active_suffixes);
/* Test support, process-wide: batch_cap / occ_segment of the wide builder inside gsa_create_from_pac (GSA_CREATE_SORT_WIDE), and active_cap -- an upper limit on
 * the entries of the wide builder's list of tied suffixes, in gsa_create_from_pac and gsa_build_index_opts alike (how a test reaches the GSA_ERR_NOMEM of a list that
 * does not fit).  0: the defaults; negative: GSA_ERR_ARG */
int gsa_set_index_build_caps(int64_t batch_cap, int64_t occ_segment, int64_t active_cap);
/* The wide builder's batch planner, a host function: hist[n_classes] suffix counts -> consecutive class ranges of at most batch_cap suffixes.  first[b] = the
 * first class of batch b, first[*n_batches] = n_classes; base[b] = 1 + the suffixes in front of batch b (its first SA slot: '$' keeps slot 0), base[*n_batches]
 * = 1 + all suffixes.  A class over the cap is a batch of its own (empty classes between two such classes form a batch of no suffix, which
 * the builder skips).  first / base hold max_batches + 1 entries.  A class of more than 2 147 483 646 suffixes: GSA_ERR_LIMIT. */
int gsa_plan_index_batches(const uint64_t *hist, int64_t n_classes, int64_t batch_cap, int64_t max_batches, int64_t *first, uint64_t *base, int64_t *n_batches);

/* ---- one long contig on several GPUs ---------------------------------------
 * IdentifyLocalMEM hands 10 000-bp chunks of the contig to whichever thread is free (GSAlign.cpp:61-94) and seeds never
 * cross a chunk edge, so the seed search of one contig splits by chunk range: every GPU runs gsa_seed_chunks on its range
 * [chunk_beg, chunk_end) of the SAME contig, the hits (sort key + length/rank word per located hit) travel to the GPU
 * that owns the contig (gsa_export_hits -> any transport -> gsa_import_hits; buffers may be host or device memory), and
 * the owner runs the rest -- SeedGrouping ... GenerateFragAlignment -- with gsa_finish_contig.  The result is the one
 * gsa_align_contig gives (hit order does not matter: the seeds are sorted next). */
int gsa_seed_chunks(gsa_ctx *ctx, const char *query, int32_t qlen, int32_t chunk_beg, int32_t chunk_end);
int64_t gsa_hit_count(gsa_ctx *ctx);
int gsa_export_hits(gsa_ctx *ctx, uint64_t *keys, uint32_t *vals);
int gsa_import_hits(gsa_ctx *ctx, const uint64_t *keys, const uint32_t *vals, int64_t n);
/* the hits of gsa_seed_chunks where they lie (device pointers, valid until the next call on ctx): same-node transport */
int gsa_hit_buffers(gsa_ctx *ctx, const uint64_t **keys, const uint32_t **vals);
int gsa_finish_contig(gsa_ctx *ctx, gsa_result *out);

/* ---- stage-level entry points (what the parity tests drive) --------------
 * gsa_set_query uploads a contig; gsa_run_to(stage) advances the same
 * eight-stage sequence the oracle uses:
 *  1 IdentifyLocalMEM + SeedGrouping            GSAlign.cpp:51-107,126-143,492-495
 *  2 GenerateAlignmentBlocks                    GSAlign.cpp:305-391,497
 *  3 CheckAlnBlockOverlaps                      ProcessCandidateAlignment.cpp:189-239
 *  4 CheckAlnBlockLargeGaps + RemoveBadAlnBlocks  :120-156,72-79 ; KmerAnalysis.cpp:78-121
 *  5 CheckAlnBlockSpanMultiSeqs + RemoveBadAlnBlocks  :81-118
 *  6 EstChromosomeSimilarity + RemoveRedundantAlnBlocks(1),(2)   GSAlign.cpp:393-471
 *  7 FillAlnBlockGaps                           ProcessCandidateAlignment.cpp:241-276
 *  8 GenerateFragAlignment + identity filter    ProcessCandidateAlignment.cpp:290-351, GSAlign.cpp:523-540
 */
/* `query` is uploaded asynchronously: the buffer must stay valid and unmodified until the next synchronising call on this
 * context returns (gsa_run_to, gsa_seed_chunks, gsa_align_contig) -- a loader may not refill a pinned buffer earlier. */
int gsa_set_query(gsa_ctx *ctx, const char *query, int32_t qlen);
int gsa_set_query_device(gsa_ctx *ctx, const char *d_query, int32_t qlen);   /* see gsa_align_contig_device */
/* back to stage 0 with the contig gsa_set_query uploaded (no new copy): the same alignment can be run again, e.g. with
 * other parameters (the reference re-reads the contig from its FASTA buffer: GSAlign.cpp:483) */
int gsa_rewind(gsa_ctx *ctx);
int gsa_run_to(gsa_ctx *ctx, int stage);

/* stage 1 outputs: SeedVec in final order, and the SeedGrouping ranges */
int64_t gsa_seed_count(gsa_ctx *ctx);
int  gsa_get_seeds(gsa_ctx *ctx, gsa_seed *out);                   /* out[gsa_seed_count] */
int  gsa_group_count(gsa_ctx *ctx);
int  gsa_get_groups(gsa_ctx *ctx, int32_t *beg, int32_t *end);
/* stage >= 2 outputs: the current AlnBlockVec */
int  gsa_get_blocks(gsa_ctx *ctx, gsa_result *out);

/* ---- leaf operators ------------------------------------------------------ */
/* BWT_Search (bwt_search.cpp:141-185) for a batch of (start, stop) windows of
 * the current query: out_len[i] = match length, out_freq[i] = accepted hit
 * count (0 if rejected), out_loc[100*i ..] = located positions. */
int gsa_bwt_search_batch(gsa_ctx *ctx, int32_t n, const int32_t *start, const int32_t *stop,
                         int32_t *out_len, int32_t *out_freq, int64_t *out_loc);

/* ksw2_alignment (ksw2_alignment.cpp:251-273) for a batch of fragment pairs:
 * s1 = reference-side fragment (length m), s2 = query-side fragment (length n),
 * given as offsets into two byte pools.  ops receives, per pair, the forward
 * M/D/I string ('D' = gap in s1, 'I' = gap in s2) at ops_off[i]; ops_len[i]
 * <= m+n.  Caller sizes ops as sum(m+n). */
int gsa_ksw2_batch(gsa_ctx *ctx, int32_t n_pairs,
                   const char *pool1, const int64_t *off1, const int32_t *len1,
                   const char *pool2, const int64_t *off2, const int32_t *len2,
                   char *ops, const int64_t *ops_off, int32_t *ops_len);

/* CalGapSimilarity (KmerAnalysis.cpp:78-121) on the current query, batch */
int gsa_gap_similarity_batch(gsa_ctx *ctx, int32_t n, const int32_t *q1, const int32_t *q2,
                             const int64_t *r1, const int64_t *r2, int32_t *similar);

/* ---- measurement ---------------------------------------------------------
 * Event counters and HIP-event timings of the last gsa_align_contig /
 * gsa_run_to sequence.  counters: [0] Occ blocks read by seed extension,
 * [1] LF steps, [2] located hits, [3] seeds, [4] DP cells, [5] DP jobs,
 * [6] sum(m+n) over DP jobs, [7] Occ blocks actually read incl. speculative walks
 * ([0] counts what the reference's walk reads = the algorithmic figure).  kernel_ms: per-kernel-family device
 * time measured with hipEvents on the library's stream:
 * [0] seed search [1] locate [2] sorts [3] chaining (S2) [4] refinement (S3-S6)
 * [5] DP + string materialisation [6] total device time [7] host list logic. */
int gsa_get_counters(gsa_ctx *ctx, uint64_t counters[8]);
int gsa_get_timings(gsa_ctx *ctx, float kernel_ms[8]);
/* Host wall clock the calling thread spent inside the library per phase, summed over the contigs aligned since the last
 * gsa_set_profiling: ms[0] query set-up (upload, or the wait for a prefetched one), ms[s] stage s = 1..8 of gsa_run_to (a stage ends
 * where the host has to look at a count: ms[1] seed search incl. its read-back ... ms[8] DP + strings + the results' D2H);
 * *n = contigs; on the context that owns the index, ms[9] / *n = mean duration of one query upload (the Uploader's copies, one at a time).
 * Always on (nine clock reads per contig). */
int gsa_get_wall_sums(gsa_ctx *ctx, double ms[10], int64_t *n);
/* What growing its buffers has cost this context since it was created: host wall time inside hipMalloc / hipHostMalloc / the frees (and the wait for
 * the context's streams in front of a free), number of allocations, bytes allocated.  A context allocates when it meets a larger contig than it has
 * seen (the reference's vectors grow the same way inside GenomeComparison, GSAlign.cpp:473-552): a steady-state loop shows no growth here. */
int gsa_get_alloc_stats(gsa_ctx *ctx, double *ms, int64_t *n, int64_t *bytes);
/* diagnosis: the `top` largest device buffers of the context to stderr (name, bytes held, bytes last asked for) */
int gsa_debug_buffers(gsa_ctx *ctx, int top);
/* flags: bit 0 = per-stage hipEvent timing; bit 1 = run the ACCOUNTING build of the seed kernel,
 * which also records, per search, how many Occ blocks the reference's walk reads, so that counters[0]
 * is exact (same seeds either way; the default build leaves counters[0] = 0); bit 2 = time the seed
 * search kernel only (kernel_ms[0]; two events per contig instead of ten); kernel_ms[6] is then the SUM of that time over
 * all contigs since the flag was set (what a benchmark divides by its contig count); bit 3 = time the gsa_call_variants passes
 * (gsa_get_variant_timing; changes nothing else: bundles stay, kernel_ms[] is not touched). */
int gsa_set_profiling(gsa_ctx *ctx, int flags);
/* How the seed search of the last contig went (IdentifyLocalMEM, GSAlign.cpp:51-107):
 * [0] most resolver rounds of a chunk, [1] chunks redone by the dense search (every start position in parallel: the
 * `freq > MaxSeedFreq` reject-and-restart regime of bwt_search.cpp:177-182, or -sen), [2] most wave-iterations of a chunk,
 * [3..5] slowest chunk: round 1 / resolver / up to the marks, in 10 ns ticks; [6..7] reserved. */
int gsa_get_seed_stats(gsa_ctx *ctx, uint64_t stats[8]);
/* What the striped gap DP launched since the context was made (sums; a clone starts at zero): [0] jobs, [1] of them side by side with a partner
 * (option "dp_pair"), [2] launches of the lagged form, [3] launches of the side-by-side form. */
int gsa_get_dp_stats(gsa_ctx *ctx, uint64_t stats[4]);
/* What the band class of the striped gap DP did since the context was made (options "dp_band", "dp_band_margin"; a clone starts at zero): [0] jobs
 * evaluated inside the diagonal band, [1] of them certified -- the band result is the full matrix's and stands --, [2] fallen back to the striped
 * kernel.  Waits for the context's work in flight. */
int gsa_get_dp_band_stats(gsa_ctx *ctx, uint64_t stats[3]);
/* The launch counters a context never resets ("Counters that are never reset"; a clone starts at zero): [0] epoch of the fused passes' look-back
 * words (30 bits), [1] the host's value of their ticket counter (32 bits, modular), [2] epoch of the striped DP's boundary granules (16 bits), [3] tag of the
 * band class's certificate flags, [4] epoch and [5] ticket value of the sliced window-chain walk, [6] slices the last sliced walk went through -- 1 + the entry
 * words that carry its epoch, read back from the device; 0 if there was none --, [7] bytes held by the boundary-granule buffer (unchanged between two calls:
 * the buffer was not replaced).  Waits for the context's work in flight and reads the two device ticket words: GSA_ERR_STATE ("ticket drift") if one differs
 * from the host's value -- the next launch of that kind would wait out its bound. */
int gsa_get_launch_counters(gsa_ctx *ctx, uint64_t v[8]);

#ifdef __cplusplus
}
#endif
#endif
