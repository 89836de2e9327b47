// gsalign_amd/csrc/host/main.cpp -- GSAlign_hip: command-line front end with the
// reference's surface (reference src/main.cpp:14-334): same flags, same defaults
// (the CODE's defaults: -clr 200, -alen 200), same output files, with the per-contig
// hot path handed to libgsa_hip.so (gsa_align_contig) instead of GenomeComparison's
// pthread stages.  Extra flags: -gpu LIST (device ordinals, comma separated: the query contigs shard over them with the
// index replicated), -ctx N (contexts per GPU: gsa_clone, contigs overlap on one device) and -timing
// (one JSON line on stderr: where the wall time of the run went).  -gpuindex: an index that has to be built (`index`, or -r) gets its BWT/SA half from the
// GPU (gsa_build_index_opts) instead of the host's suffix sorters; the files are the same bytes.  -memindex (with -r): no index file at all -- the reference FASTA is
// parsed (gsah_reference_from_fasta) and the first GPU's context is made from its .pac bytes in device memory (gsa_create_from_pac).  -lift FILE: the reference positions
// listed in FILE (name, 1-based position; a VCF works as it is) are carried through every contig's alignment on the GPU (gsa_lift) and written to <prefix>.lift.tsv.  -liftbed FILE: the reference
// intervals of FILE (BED) are carried through every contig's alignment on the GPU (gsa_lift_regions) and written with their class counts to <prefix>.regions.tsv.
// -track W: the reference sequences in windows of W bases -- covered, matching, mismatching, deleted and inserted bases per window and query contig, computed on the GPU
// (gsa_ref_track) and written to <prefix>.track.tsv.  -qtrack W: the mirror image -- every query contig in windows of W bases: covered, multiply covered, matching,
// mismatching, inserted and deleted bases per window (gsa_query_track), written to <prefix>.qtrack.tsv.  -proj: the query in reference coordinates -- one character per reference base over all
// query contigs, painted on the GPU into one accumulator per device (gsa_project) and written to <prefix>.proj.fa.  -chain: every alignment as a UCSC chain (for liftOver, CrossMap, bcftools +liftover), its size / dt / dq lines
// computed on the GPU (gsa_block_segs) and written to <prefix>.chain.
// The contigs go through gsa_align_many (the per-contig loop of GSAlign.cpp:483-548).  Round 5: a GPU worker thread only COPIES a finished
// contig out of the library's memory; ONE formatter thread takes the contigs in contig order (OutputMAF appends per contig, VarVec grows in
// contig order: GSAlign.cpp:543-546) and formats each with the host pool's threads (par.h: the text lines of a block, the variants of a
// block's records), a writer thread writes the buffers in order -- so the output bytes depend neither on GPUs / contexts nor on -t.
#include <errno.h>
#include <malloc.h>
#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <fcntl.h>
#include <unistd.h>
#include "gsa_host.h"
#include "par.h"

static void usage(const char *prog, int t, const gsa_params &p, int fmt)
{
	fprintf(stderr, "\nGenAlign v%s\n", "1.0.22");
	fprintf(stderr, "Usage: %s [-i IndexFile Prefix / -r Reference file] -q QueryFile[Fasta]\n\n", prog);
	fprintf(stderr, "Options: -t     INT     number of threads [%d] (host side: FASTA / index loading, MAF / VCF formatting; the hot path runs on the GPU)\n", t);
	fprintf(stderr, "         -o     STR     Set the prefix of the output files [output]\n");
	fprintf(stderr, "         -fmt   INT     Set the output format 1:maf, 2:aln, 3:paf [%d]\n", fmt);
	fprintf(stderr, "         -idy   INT     Set the minimal sequence identity (0-100) of a local alignment [%d]\n", p.min_identity);
	fprintf(stderr, "         -slen  INT     Set the minimal seed length [%d]\n", p.min_seed_len);
	fprintf(stderr, "         -alen  INT     Set the minimal alignment length [%d]\n", p.min_aln_len);
	fprintf(stderr, "         -ind   INT     Set the maximal indel size [%d]\n", p.max_indel);
	fprintf(stderr, "         -clr   INT     Set the minimal cluster size [%d]\n", p.min_block_score);
	fprintf(stderr, "         -unique        Output unique alignment only [false]\n");
	fprintf(stderr, "         -sen           Sensitive mode [False]\n");
	fprintf(stderr, "         -dp            Output Dot-plots\n");
	fprintf(stderr, "         -one           set one on one aligment mode[false]\n");
	fprintf(stderr, "         -gp    STR     Specify the path of gnuplot\n");
	fprintf(stderr, "         -no_vcf        do not write the VCF file\n");
	fprintf(stderr, "         -gpu   LIST    GPU ordinals, comma separated [0]\n");
	fprintf(stderr, "         -ctx   INT     contexts per GPU working on different query sequences [2]\n");
	fprintf(stderr, "         -timing        print where the wall time went (one JSON line on stderr)\n");
	fprintf(stderr, "         -cs            with -fmt 3: add the cs:Z: difference string (short form) of every alignment, computed on the GPU (gsa_block_cs) [false]\n");
	fprintf(stderr, "         -lift  FILE    lift the reference positions of FILE (tab-separated: sequence name, 1-based position; '#' lines skipped, a VCF works) to the query on the GPU (gsa_lift): <prefix>.lift.tsv\n");
	fprintf(stderr, "         -proj          project the query onto the reference on the GPU (gsa_project): one character per reference base over all query sequences -- the aligned query base, '-' deleted, 'n' not aligned: <prefix>.proj.fa\n");
	fprintf(stderr, "         -track INT     per window of INT reference bases and query sequence: covered / matching / mismatching / deleted / inserted bases, computed on the GPU (gsa_ref_track): <prefix>.track.tsv\n");
	fprintf(stderr, "         -qtrack INT    per window of INT bases of every query sequence: covered / multiply covered / matching / mismatching / inserted / deleted bases, computed on the GPU (gsa_query_track): <prefix>.qtrack.tsv\n");
	fprintf(stderr, "         -liftbed FILE  lift the reference intervals of FILE (BED: sequence name, 0-based start, end, optional name) to the query on the GPU (gsa_lift_regions), with match / mismatch / deleted / inserted counts: <prefix>.regions.tsv\n");
	fprintf(stderr, "         -chain         write every alignment as a UCSC chain (liftOver, CrossMap), its segments computed on the GPU (gsa_block_segs): <prefix>.chain [false]\n");
	fprintf(stderr, "         -gpuvar        identify the sequence variants on the GPU (gsa_call_variants) instead of on the host [false]\n");
	fprintf(stderr, "         -gpuindex      build the index (-r, or `%s index [-gpuindex] [-gpu N] ref.fa prefix`) on the GPU (gsa_build_index_opts; over 1.07 Gbp its batched 64-bit sorter) [false]\n", prog);
	fprintf(stderr, "         -memindex      with -r: build the index in GPU memory (gsa_create_from_pac) and align against it; no index file is written or read (over 1.07 Gbp: the batched 64-bit sorter) [false]\n\n");
}

// GSA_INDEX_64BIT=1: the wide device builder on any input (as it forces the wide host sorter); GSA_INDEX_BATCH=N: its batch cap (how the tests reach several batches with a small fixture)
static bool env_index_wide() { const char *e = getenv("GSA_INDEX_64BIT"); return e && *e && *e != '0'; }
static int64_t env_index_batch() { const char *e = getenv("GSA_INDEX_BATCH"); const long long v = e ? atoll(e) : 0; return v > 0 ? v : 0; }
// the index of `fasta` under `prefix`; on_gpu: the BWT/SA half from gsa_build_index_opts on `device` (GSA_BUILD_AUTO: the wide sorter over 1 073 741 822 bases; a reference
// over ITS bound: one line, then the host builder).  Returns 0, 1 (the builder's error: printed) or 2 (the GPU's error: printed).
struct GpuIndexCall { int device, rc; };
static int gpu_bwt_fn(void *user, const uint8_t *pac, int64_t G, uint64_t *primary, uint64_t L2[5], uint32_t *bwt, uint64_t *sa)
{
	GpuIndexCall *g = (GpuIndexCall *)user;
	return g->rc = gsa_build_index_opts(g->device, pac, G, env_index_wide() ? GSA_BUILD_WIDE : GSA_BUILD_AUTO, env_index_batch(), 0, primary, L2, bwt, sa);
}
static int build_index(const char *fasta, const std::string &prefix, bool on_gpu, int device)
{
	std::string e;
	if (on_gpu) {
		GpuIndexCall g = { device, GSA_OK };
		if (gsah_build_index_with(fasta, prefix, e, gpu_bwt_fn, &g)) return 0;
		if (g.rc == GSA_OK) { fprintf(stderr, "%s\n", e.c_str()); return 1; }
		if (g.rc != GSA_ERR_LIMIT) { fprintf(stderr, "GPU index build failed (device %d): %s\n", device, gsa_last_error(NULL)); return 2; }
		fprintf(stderr, "-gpuindex: %s; building the index on the host\n", gsa_last_error(NULL));
	}
	if (!gsah_build_index(fasta, prefix, e)) { fprintf(stderr, "%s\n", e.c_str()); return 1; }
	return 0;
}

static bool check_prefix(const char *p)                     // CheckOutputPrefix (main.cpp:116-138)
{
	if (strcmp(p, "/dev/null") == 0) return true;
	for (size_t i = 0; i < strlen(p); i++) {
		const int c = (unsigned char)p[i];
		if (!isprint(c) || (c >= 32 && c <= 44) || (c >= 58 && c <= 64) || (c >= 123 && c <= 127)) { fprintf(stderr, "FatalError: Please specify a valid prefix name\n"); return false; }
	}
	return true;
}

static bool first_char_is_header(const char *path)          // CheckInputFile (main.cpp:49-64)
{
	FILE *fp = fopen(path, "r"); if (!fp) return false;
	int c = fgetc(fp); fclose(fp);
	return c == '>';
}

// -lift FILE: name <tab> 1-based position [<tab> anything]; '#' lines and empty lines are skipped.  pos: 0-based forward global coordinates, chr / at: sequence and 1-based
// position of every entry.  false: one line on stderr (the file, an unknown name, a position outside its sequence)
static bool load_lift_file(const char *path, const HostIndex &idx, std::vector<int64_t> &pos, std::vector<int32_t> &chr, std::vector<int32_t> &at)
{
	FILE *fp = fopen(path, "r");
	if (!fp) { fprintf(stderr, "-lift: cannot open %s\n", path); return false; }
	std::string line; long long ln = 0; bool ok = true;
	for (int ch = 0; ok && ch != EOF;) {
		line.clear();
		while ((ch = fgetc(fp)) != EOF && ch != '\n') line.push_back((char)ch);
		ln++;
		if (!line.empty() && line[line.size() - 1] == '\r') line.resize(line.size() - 1);
		if (line.empty() || line[0] == '#') continue;
		const size_t t1 = line.find('\t');
		const std::string name = line.substr(0, t1);
		char *end = nullptr;
		const long long p1 = t1 == std::string::npos ? 0 : strtoll(line.c_str() + t1 + 1, &end, 10);
		if (t1 == std::string::npos || end == line.c_str() + t1 + 1) { fprintf(stderr, "-lift: %s line %lld: expected a sequence name, a tab and a position\n", path, ln); ok = false; break; }
		size_t c = 0; while (c < idx.chr_name.size() && idx.chr_name[c] != name) c++;
		if (c == idx.chr_name.size()) { fprintf(stderr, "-lift: %s line %lld: unknown reference sequence %s\n", path, ln, name.c_str()); ok = false; break; }
		if (p1 < 1 || p1 > idx.chr_len[c]) { fprintf(stderr, "-lift: %s line %lld: position %lld lies outside %s (1 .. %d)\n", path, ln, p1, name.c_str(), idx.chr_len[c]); ok = false; break; }
		pos.push_back(idx.chr_fwd[c] + p1 - 1); chr.push_back((int32_t)c); at.push_back((int32_t)p1);
	}
	fclose(fp);
	return ok;
}

// -liftbed FILE: BED -- name <tab> 0-based start <tab> end [<tab> region name [<tab> anything]]; '#', "track", "browser" and empty lines are skipped.  beg / end: 0-based
// forward global coordinates, chr / lo / hi: sequence and local interval of every entry, name: its 4th column ("." when absent).  false: one line on stderr (the file,
// a malformed line, an unknown name, start >= end, an end beyond its sequence)
static bool load_bed_file(const char *path, const HostIndex &idx, std::vector<int64_t> &beg, std::vector<int64_t> &end, std::vector<int32_t> &chr, std::vector<int32_t> &lo,
                          std::vector<int32_t> &hi, std::vector<std::string> &name)
{
	FILE *fp = fopen(path, "r");
	if (!fp) { fprintf(stderr, "-liftbed: cannot open %s\n", path); return false; }
	std::string line; long long ln = 0; bool ok = true;
	for (int ch = 0; ok && ch != EOF;) {
		line.clear();
		while ((ch = fgetc(fp)) != EOF && ch != '\n') line.push_back((char)ch);
		ln++;
		if (!line.empty() && line[line.size() - 1] == '\r') line.resize(line.size() - 1);
		if (line.empty() || line[0] == '#' || line.compare(0, 5, "track") == 0 || line.compare(0, 7, "browser") == 0) continue;
		const size_t t1 = line.find('\t'), t2 = t1 == std::string::npos ? t1 : line.find('\t', t1 + 1);
		char *e1 = nullptr, *e2 = nullptr;
		const long long p0 = t2 == std::string::npos ? 0 : strtoll(line.c_str() + t1 + 1, &e1, 10), p1 = t2 == std::string::npos ? 0 : strtoll(line.c_str() + t2 + 1, &e2, 10);
		if (t2 == std::string::npos || e1 != line.c_str() + t2 || e1 == line.c_str() + t1 + 1 || e2 == line.c_str() + t2 + 1 || (*e2 != 0 && *e2 != '\t')) {
			fprintf(stderr, "-liftbed: %s line %lld: expected a sequence name, a start and an end, tab-separated\n", path, ln); ok = false; break;
		}
		const std::string sname = line.substr(0, t1);
		size_t c = 0; while (c < idx.chr_name.size() && idx.chr_name[c] != sname) c++;
		if (c == idx.chr_name.size()) { fprintf(stderr, "-liftbed: %s line %lld: unknown reference sequence %s\n", path, ln, sname.c_str()); ok = false; break; }
		if (p0 < 0 || p0 >= p1) { fprintf(stderr, "-liftbed: %s line %lld: start %lld is not below end %lld\n", path, ln, p0, p1); ok = false; break; }
		if (p1 > idx.chr_len[c]) { fprintf(stderr, "-liftbed: %s line %lld: end %lld lies beyond %s (%d bases)\n", path, ln, p1, sname.c_str(), idx.chr_len[c]); ok = false; break; }
		std::string nm = ".";
		if (*e2 == '\t') { const size_t a = (size_t)(e2 - line.c_str()) + 1, z = line.find('\t', a); if (z != a && a < line.size()) nm = line.substr(a, z == std::string::npos ? z : z - a); }
		beg.push_back(idx.chr_fwd[c] + p0); end.push_back(idx.chr_fwd[c] + p1); chr.push_back((int32_t)c); lo.push_back((int32_t)p0); hi.push_back((int32_t)p1); name.push_back(nm);
	}
	fclose(fp);
	return ok;
}

static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int main(int argc, char *argv[])
{
	// -ctx contexts x 5 streams each; the runtime's default is 4 hardware queues per process.  bench.py uses the same value (--hwq); see INTEGRATION.md
	setenv("GPU_MAX_HW_QUEUES", "16", 0);
	// (finished contigs are copied into fresh ~100 MB blocks and freed after they are written: keep that memory in the heap instead of handing it back to the
	//  kernel and faulting it in again for the next contig)
	mallopt(M_MMAP_THRESHOLD, 1 << 30); mallopt(M_TRIM_THRESHOLD, 1 << 30); mallopt(M_TOP_PAD, 256 << 20);
	gsa_params prm; gsa_default_params(&prm);
	int threads = HostPool::default_threads(), fmt = 1, n_ctx_per_gpu = 2; bool vcf = true, allow_dup = true, dotplot = false, gpuvar = false, want_cs = false, want_chain = false, want_proj = false, gpuindex = false, memindex = false, timing = getenv("GSA_TIMING") != NULL;
	std::vector<int> gpus;
	const char *index_prefix = NULL, *ref_fa = NULL, *query_fa = NULL, *out_prefix = NULL, *gnuplot_arg = NULL, *lift_file = NULL, *bed_file = NULL;
	int track_w = 0;      // -track W (0: no track)
	int qtrack_w = 0;     // -qtrack W (0: no query track)
	if (argc == 1 || strcmp(argv[1], "-h") == 0) { usage(argv[0], threads, prm, fmt); return 0; }
	if (strcmp(argv[1], "index") == 0) {
		bool on_gpu = false; int device = 0, a = 2;
		for (; a < argc && argv[a][0] == '-'; a++) { if (strcmp(argv[a], "-gpuindex") == 0) on_gpu = true; else if (strcmp(argv[a], "-gpu") == 0 && a + 1 < argc) device = atoi(argv[++a]); else break; }
		if (argc - a == 2) return build_index(argv[a], argv[a + 1], on_gpu, device);
		fprintf(stderr, "usage: %s index [-gpuindex] [-gpu N] ref.fa prefix\n", argv[0]);
		return 0;
	}
	for (int i = 1; i < argc; i++) {
		const std::string a = argv[i];
		if (a == "-i") index_prefix = argv[++i];
		else if (a == "-r" && i + 1 < argc) ref_fa = argv[++i];
		else if (a == "-q" && i + 1 < argc) query_fa = argv[++i];
		else if (a == "-t" && i + 1 < argc) { if ((threads = atoi(argv[++i])) < 0) { fprintf(stderr, "Warning! Thread number should be greater than 0!\n"); threads = 16; } }
		else if (a == "-slen" && i + 1 < argc) { prm.min_seed_len = atoi(argv[++i]); if (prm.min_seed_len < 10 || prm.min_seed_len > 30) { fprintf(stderr, "Warning! minimal seed length is between 10~20!\n"); return 0; } }
		else if (a == "-ind" && i + 1 < argc) { prm.max_indel = atoi(argv[++i]); if (prm.max_indel < 10 || prm.max_indel > 100) { fprintf(stderr, "Warning! maximal indel size is between 10~100!\n"); return 0; } }
		else if (a == "-sen" || a == "-sensitive") { prm.sensitive = 1; prm.min_aln_len = 200; prm.min_block_score = 50; }
		else if (a == "-unique") allow_dup = false;
		else if (a == "-no_vcf") vcf = false;
		else if (a == "-one") prm.one_on_one = 1;
		else if (a == "-idy" && i + 1 < argc) prm.min_identity = atoi(argv[++i]);
		else if (a == "-alen" && i + 1 < argc) prm.min_aln_len = atoi(argv[++i]);
		else if (a == "-clr" && i + 1 < argc) prm.min_block_score = atoi(argv[++i]);
		else if (a == "-fmt" && i + 1 < argc) fmt = atoi(argv[++i]);
		else if (a == "-o") out_prefix = argv[++i];
		else if (a == "-gpu" && i + 1 < argc) { for (const char *p = argv[++i]; *p;) { gpus.push_back(atoi(p)); while (*p && *p != ',') p++; if (*p == ',') p++; } }
		else if (a == "-ctx" && i + 1 < argc) { n_ctx_per_gpu = atoi(argv[++i]); if (n_ctx_per_gpu < 1) n_ctx_per_gpu = 1; }
		else if (a == "-timing") timing = true;
		else if (a == "-gpuvar") gpuvar = true;
		else if (a == "-cs") want_cs = true;
		else if (a == "-chain") want_chain = true;
		else if (a == "-proj") want_proj = true;
		else if (a == "-lift" && i + 1 < argc) lift_file = argv[++i];
		else if (a == "-liftbed" && i + 1 < argc) bed_file = argv[++i];
		else if (a == "-track" && i + 1 < argc) {
			char *end = NULL; const long long w = strtoll(argv[++i], &end, 10);
			if (end == argv[i] || *end || w < 1 || w > 0x7fffffffll) { fprintf(stderr, "-track: the window must be a number of bases from 1 to 2147483647 (got %s)\n", argv[i]); return 1; }
			track_w = (int)w;
		}
		else if (a == "-qtrack" && i + 1 < argc) {
			char *end = NULL; const long long w = strtoll(argv[++i], &end, 10);
			if (end == argv[i] || *end || w < 1 || w > 0x7fffffffll) { fprintf(stderr, "-qtrack: the window must be a number of bases from 1 to 2147483647 (got %s)\n", argv[i]); return 1; }
			qtrack_w = (int)w;
		}
		else if (a == "-gpuindex") gpuindex = true;
		else if (a == "-memindex") memindex = true;
		else if (a == "-dp") dotplot = true;
		else if (a == "-gp" && i + 1 < argc) gnuplot_arg = argv[++i];      // main.cpp:285: the path of gnuplot, used as given
		else if (a == "-d" || a == "-debug") { /* debug printers: not reproduced */ }
		else if (a == "-obr" && i + 1 < argc) ++i;
		else fprintf(stderr, "Warning! Unknow parameter: %s\n", argv[i]);
	}
	if ((index_prefix == NULL && ref_fa == NULL) || query_fa == NULL) { usage(argv[0], threads, prm, fmt); return 0; }
	if (out_prefix == NULL) out_prefix = "output"; else if (!check_prefix(out_prefix)) return 0;
	if (want_cs && fmt != 3) { fprintf(stderr, "Warning! -cs adds the cs:Z: field to PAF lines (-fmt 3) only: ignored\n"); want_cs = false; }
	HostPool::global().resize(threads < 1 ? 1 : (threads > 256 ? 256 : threads));

	const time_t t0 = time(NULL);
	const double T0 = now_s();
	double t_query = 0, t_index = 0, t_create = 0, t_align = 0, t_drain = 0, t_vcf = 0, t_maf_fmt = 0, t_var = 0, t_copy = 0, t_build = 0, t_ref_parse = 0, t_from_pac = 0;
	fprintf(stderr, "Step1. Load the two genome sequences...\n");
	std::string err, qerr; std::vector<QueryContig> qs; bool q_ok = false;
	if (!first_char_is_header(query_fa)) { fprintf(stderr, "Please check the query file: %s\n", query_fa); return 0; }
	// the query FASTA is read beside the index (both use the pool: their parallel sections take turns) and beside gsa_create, which is GPU work
	std::thread q_loader([&] { const double t = now_s(); q_ok = gsah_load_query(query_fa, qs, qerr); t_query = now_s() - t; });
	struct Joiner { std::thread &t; ~Joiner() { if (t.joinable()) t.join(); } } q_join{ q_loader };
	HostIndex idx; std::string prefix;
	if (index_prefix != NULL && gsah_index_files_exist(index_prefix)) {
		prefix = index_prefix;
		if (memindex) { fprintf(stderr, "-memindex: the index files of %s exist and are used\n", index_prefix); memindex = false; }
	} else if (ref_fa != NULL && first_char_is_header(ref_fa) && memindex) {
		// the FASTA half of the index builder only: names, lengths and the .pac bytes stay in memory, nothing is written beside the reference
		const double t = now_s(); const bool ok = gsah_reference_from_fasta(ref_fa, idx, err); t_ref_parse = now_s() - t;
		if (!ok) { fprintf(stderr, "%s\n", err.c_str()); return 1; }
	} else if (ref_fa != NULL && first_char_is_header(ref_fa)) {
		prefix = ref_fa; size_t p = prefix.find_last_of('.'); if (p != std::string::npos && p > 0) prefix.resize(p);
		const double t = now_s();
		if (const int rcb = build_index(ref_fa, prefix, gpuindex, gpus.empty() ? 0 : gpus[0])) return rcb;
		t_build = now_s() - t;
	} else { q_loader.join(); if (!q_ok) fprintf(stderr, "Please check the query file: %s\n", query_fa); else fprintf(stderr, "Please specify a valid reference genome\n"); return 0; }
	// while the files are read: the HIP runtime comes up and the device memory of the two largest tables (their sizes follow from the text length in the .bwt header)
	// is set aside -- ~0.4 s of hipMalloc for a human index that gsa_create would otherwise spend AFTER the files are in
	if (gpus.empty()) gpus.push_back(0);
	double t_reserve = 0, t_reserve_wait = 0, t_unpack_wait = 0, t_at_align = 0;
	std::thread reserver([&] {
		if (memindex) return;      // (no .bwt header to read the text length from, and gsa_create_from_pac adopts no reservation)
		if (lift_file || bed_file) return;     // (-lift, -liftbed: no GPU work before the position file has been checked against the reference's sequence table, which needs the index files)
		const double t = now_s();
		uint64_t hdr[5] = { 0, 0, 0, 0, 0 };
		FILE *fb = fopen((prefix + ".bwt").c_str(), "rb");
		const bool ok = fb && fread(hdr, 8, 5, fb) == 5; if (fb) fclose(fb);
		const char *fw = getenv("GSA_FORCE_WIDE");
		if (ok && hdr[4] > 0) (void)gsa_reserve_index(gpus[0], hdr[4], (fw && *fw && *fw != '0') ? GSA_CREATE_WIDE : 0u);
		t_reserve = now_s() - t;
	});
	struct Joiner3 { std::thread &t; ~Joiner3() { if (t.joinable()) t.join(); } } reserve_join{ reserver };
	// the index files as they lie on disk first (.bwt, .sa, .ann, the raw .pac bytes); RefSequence -- which only the emitters of THIS program read -- is unpacked further
	// down, beside gsa_create: the device gets the .pac bytes and unpacks its own copy (GSA_CREATE_REF_PAC)
	if (!memindex) { const double t = now_s(); const bool ok = gsah_load_index_files(prefix, idx, err); t_index = now_s() - t; if (!ok) { fprintf(stderr, "\n\nError! Please check your input! (%s)\n", err.c_str()); return 1; } }

	// -lift: the positions are checked against the reference's sequence table before any context exists
	std::vector<int64_t> lift_pos; std::vector<int32_t> lift_chr, lift_at;
	if (lift_file && !load_lift_file(lift_file, idx, lift_pos, lift_chr, lift_at)) return 1;
	const bool want_lift = lift_file != NULL && !lift_pos.empty();
	if (lift_file && !want_lift) fprintf(stderr, "Warning! -lift: %s holds no position\n", lift_file);

	// -liftbed: the same for the regions
	std::vector<int64_t> bed_beg, bed_end; std::vector<int32_t> bed_chr, bed_lo, bed_hi; std::vector<std::string> bed_name;
	if (bed_file && !load_bed_file(bed_file, idx, bed_beg, bed_end, bed_chr, bed_lo, bed_hi, bed_name)) return 1;
	const bool want_regions = bed_file != NULL && !bed_beg.empty();
	if (bed_file && !want_regions) fprintf(stderr, "Warning! -liftbed: %s holds no region\n", bed_file);

	// FindGnuPlotPath (main.cpp:169-191): -dp needs a gnuplot binary -- the one -gp names, else the first one on PATH; without one the
	// reference plots nothing either
	std::string gnuplot = gnuplot_arg ? gnuplot_arg : "";
	if (dotplot && gnuplot.empty()) {
		const char *path = getenv("PATH");
		for (std::string p = path ? path : ""; !p.empty();) {
			const size_t k = p.find(':'); const std::string dir = p.substr(0, k);
			FILE *fp = fopen((dir + "/gnuplot").c_str(), "r");
			if (fp) { fclose(fp); gnuplot = dir + "/gnuplot"; break; }
			if (k == std::string::npos) break;
			p = p.substr(k + 1);
		}
	}
	gsa_index_view view; idx.fill_view(&view);
	view.ref = (const char *)idx.pac.data();      // (GSA_CREATE_REF_PAC below)
	if (gpus.empty()) gpus.push_back(0);
	double t_unpack = 0; bool unpack_ok = false; std::string unpack_err;
	std::thread unpacker([&] { const double t = now_s(); unpack_ok = gsah_unpack_ref(idx, unpack_err, true); t_unpack = now_s() - t; });      // (RestoreReferenceInfo for the emitters, beside gsa_create)
	struct Joiner2 { std::thread &t; ~Joiner2() { if (t.joinable()) t.join(); } } unpack_join{ unpacker };
	if (getenv("GSA_BIND")) (void)gsa_bind_host_thread(gpus[0]);      // (opt-in: small contigs gain from a near-socket thread, chromosome-sized ones lose 5 %)
	// one context per GPU owns that device's copy of the index; the others borrow it (gsa_clone).  The number of contexts wanted depends on
	// the number of query sequences: the owners are created first (GPU work, beside the FASTA loader), the clones once the count is known
	std::vector<gsa_ctx *> ctxs;
	{ const double t = now_s(); reserver.join(); t_reserve_wait = now_s() - t; }
	{
		const double t = now_s();
		for (size_t g = 0; g < gpus.size(); g++) {
			gsa_ctx *owner = NULL;
			// (the HOST PROGRAM honours a few environment variables and hands them to the library as options -- the library itself reads none:
			//  GSA_FORCE_WIDE=1: the >= 2^32-row device layout on any index; GSA_SPLIT_MIN / GSA_BUNDLE_CONTIG / GSA_BUNDLE_CAP: gsa_align_many's policy)
			const char *fw = getenv("GSA_FORCE_WIDE");
			// (the first GPU gets the index from the host -- upload + table builds; every further GPU gets a device-to-device copy of the finished tables:
			//  gsa_clone_to_device, no second pass over PCIe, nothing rebuilt)
			const uint32_t wide = (fw && *fw && *fw != '0') ? GSA_CREATE_WIDE : 0u;
			// (-memindex: the wide sorter over the narrow one's bound of 1 073 741 822 bases, or when GSA_INDEX_64BIT asks for it)
			const uint32_t sort_wide = memindex && (env_index_wide() || idx.G > 1073741822ll) ? GSA_CREATE_SORT_WIDE : 0u;
			if (sort_wide) (void)gsa_set_index_build_caps(env_index_batch(), 0, 0);
			const double tc = now_s();
			const int rc_c = g > 0 ? gsa_clone_to_device(ctxs[0], gpus[g], &owner)
			               : memindex ? gsa_create_from_pac(gpus[g], idx.pac.data(), idx.G, idx.chr_len.data(), (int32_t)idx.chr_len.size(), &prm, wide | sort_wide, &owner)
			                          : gsa_create_opts(gpus[g], &view, &prm, wide | GSA_CREATE_REF_PAC, &owner);
			if (g == 0 && memindex) t_from_pac = now_s() - tc;
			// (a reference over the device builder's bound: the library's message, and no fall-back to a path that writes the files the user asked not to have)
			if (rc_c == GSA_ERR_LIMIT && g == 0 && memindex) { fprintf(stderr, "-memindex: %s\n", gsa_last_error(NULL)); return 1; }
			if (rc_c != GSA_OK) { fprintf(stderr, "GPU initialisation failed (device %d): %s\n", gpus[g], gsa_last_error(NULL)); return 2; }
			for (const char *nm : { "split_min", "bundle_contig", "bundle_cap" }) {
				std::string ev = std::string("GSA_") + nm; for (char &ch : ev) ch = (char)toupper((unsigned char)ch);
				if (const char *v = getenv(ev.c_str())) (void)gsa_set_option(owner, nm, atoll(v));
			}
			ctxs.push_back(owner);
		}
		t_create = now_s() - t;
	}
	{ const double t = now_s(); unpacker.join(); t_unpack_wait = now_s() - t; }
	if (!unpack_ok) { fprintf(stderr, "\n\nError! Please check your input! (%s)\n", unpack_err.c_str()); return 1; }
	idx.pac.resize(0);
	q_loader.join();
	if (!q_ok) { fprintf(stderr, "Please check the query file: %s\n", query_fa); return 0; }
	fprintf(stderr, "\tLoad the query sequences (%d %s)\n", (int)qs.size(), qs.size() > 1 ? "chromosomes" : "chromosome");
	fprintf(stderr, "\tLoad the reference sequences (%d %s)\n", (int)idx.chr_len.size(), idx.chr_len.size() > 1 ? "chromosomes" : "chromosome");
	{
		// (at least one context per listed GPU: with fewer query sequences than GPUs gsa_align_many seeds a long sequence on several of them)
		const size_t want_ctx = std::min(std::max(qs.size(), gpus.size()), gpus.size() * (size_t)n_ctx_per_gpu);
		const double t = now_s();
		for (int k = 1; k < n_ctx_per_gpu; k++)
			for (size_t g = 0; g < gpus.size() && ctxs.size() < want_ctx; g++) {
				gsa_ctx *cl = NULL;
				if (gsa_clone(ctxs[g], &cl) != GSA_OK) { fprintf(stderr, "GPU initialisation failed (device %d): %s\n", gpus[g], gsa_last_error(NULL)); return 2; }
				ctxs.push_back(cl);
			}
		t_create += now_s() - t;
	}
	// (the positions go to every context, the clones included: a clone starts without)
	if (track_w) for (gsa_ctx *c : ctxs) if (gsa_track_set(c, track_w) != GSA_OK) { fprintf(stderr, "-track: %s\n", gsa_last_error(c)); return 2; }
	if (qtrack_w) for (gsa_ctx *c : ctxs) if (gsa_qtrack_set(c, qtrack_w) != GSA_OK) { fprintf(stderr, "-qtrack: %s\n", gsa_last_error(c)); return 2; }
	// -proj: one accumulator per GPU -- its first context opens it, the clones on that GPU paint into the same array (without the duplicates under -unique)
	if (want_proj) for (size_t i = 0; i < ctxs.size(); i++) {
		gsa_ctx *first = i < gpus.size() ? NULL : ctxs[(i - gpus.size()) % gpus.size()];
		if (gsa_proj_open(ctxs[i], first, allow_dup ? 0u : GSA_PROJ_NO_DUP) != GSA_OK) { fprintf(stderr, "-proj: %s\n", gsa_last_error(ctxs[i])); return 2; }
	}
	if (want_lift) for (gsa_ctx *c : ctxs) if (gsa_lift_set(c, lift_pos.data(), (int64_t)lift_pos.size()) != GSA_OK) { fprintf(stderr, "-lift: %s\n", gsa_last_error(c)); return 2; }

	if (want_regions) for (gsa_ctx *c : ctxs) if (gsa_regions_set(c, bed_beg.data(), bed_end.data(), (int64_t)bed_beg.size()) != GSA_OK) { fprintf(stderr, "-liftbed: %s\n", gsa_last_error(c)); return 2; }

	const std::string regn = std::string(out_prefix) + ".regions.tsv";
	const std::string maf = std::string(out_prefix) + (fmt == 3 ? ".paf" : ".maf"), aln = std::string(out_prefix) + ".aln", vcfn = std::string(out_prefix) + ".vcf", liftn = std::string(out_prefix) + ".lift.tsv", trackn = std::string(out_prefix) + ".track.tsv", qtrackn = std::string(out_prefix) + ".qtrack.tsv", chainn = std::string(out_prefix) + ".chain", projn = std::string(out_prefix) + ".proj.fa";
	Emitter em; em.idx = &idx; em.allow_dup = allow_dup;
	long long n_aln = 0, tot_len = 0, tot_match = 0, n_dup = 0;
	fprintf(stderr, "Step2. Sequence analysis for all query chromosomes\n");
	std::vector<const char *> qptr(qs.size()); std::vector<int32_t> qlen(qs.size());
	for (size_t ci = 0; ci < qs.size(); ci++) { qptr[ci] = qs[ci].seq.data(); qlen[ci] = (int32_t)qs[ci].seq.size(); }
	// the sequences are page-locked where the loader put them (10 ms per GB): their uploads are DMA transfers instead of staged copies
	double t_pin = 0;
	{ const double t = now_s(); for (size_t ci = 0; ci < qs.size(); ci++) if (qs[ci].seq.size() >= ((size_t)1 << 20)) (void)gsa_host_register(&qs[ci].seq[0], qs[ci].seq.size()); t_pin = now_s() - t; }
	// finished contigs: copied by the GPU worker that produced them (on_result), taken in contig order by the formatter thread
	struct Sink {
		std::mutex mu; std::condition_variable cv; std::vector<ContigResult> res; std::vector<char> ready; bool abort = false; double copy_s = 0;
		std::vector<RawArr<gsa_variant> > var;      // -gpuvar: the contig's variants as gsa_call_variants left them
		bool want_cig = false; std::vector<RawArr<gsa_block_cigar> > cblk; std::vector<RawArr<uint32_t> > cops;      // -fmt 3: the contig's CIGARs as gsa_block_cigars left them
		std::vector<RawArr<gsa_cs_block> > sblk; std::vector<RawArr<char> > sbytes; bool want_cs = false;      // -cs: the contig's cs strings as gsa_block_cs left them
		std::vector<RawArr<gsa_lift_hit> > lift; bool want_lift = false;      // -lift: the contig's hits as gsa_lift left them
		std::vector<RawArr<gsa_region_hit> > regions; bool want_regions = false;      // -liftbed: the contig's hits as gsa_lift_regions left them
		std::vector<RawArr<gsa_qtrack_win> > qtrack; bool want_qtrack = false;   // -qtrack: the contig's windows as gsa_query_track left them
		std::vector<RawArr<gsa_track_win> > track; bool want_track = false;   // -track: the contig's windows as gsa_ref_track left them
		std::vector<RawArr<gsa_seg_block> > gblk; std::vector<RawArr<gsa_seg> > gseg; bool want_segs = false;   // -chain: the contig's triples as gsa_block_segs left them
	} sink;
	sink.res.resize(qs.size()); sink.ready.assign(qs.size(), 0); sink.var.resize(qs.size()); sink.cblk.resize(qs.size()); sink.cops.resize(qs.size()); sink.sblk.resize(qs.size()); sink.sbytes.resize(qs.size()); sink.want_cs = want_cs; sink.want_cig = fmt == 3; sink.lift.resize(qs.size()); sink.want_lift = want_lift; sink.track.resize(qs.size()); sink.want_track = track_w != 0; sink.qtrack.resize(qs.size()); sink.want_qtrack = qtrack_w != 0;
	sink.gblk.resize(qs.size()); sink.gseg.resize(qs.size()); sink.want_segs = want_chain; sink.regions.resize(qs.size()); sink.want_regions = want_regions;
	const bool var_on_gpu = gpuvar && vcf;          // (-no_vcf: nobody reads the variants)
	// the MAF file: created by the first contig that has alignments ("w" for contig 0, "a" afterwards: tools.cpp:158-163 -- a run whose
	// first contig aligns nowhere appends to whatever the file held, as the reference does)
	int maf_fd = -1; std::unique_ptr<OrderedWriter> maf_w;
	bool out_failed = false;          // an output file that could not be opened or written: reported, exit status 1 (a full disk must not look like success)
	size_t written = 0;
	FILE *lift_fp = NULL;
	if (want_lift && !(lift_fp = fopen(liftn.c_str(), "w"))) { out_failed = true; fprintf(stderr, "Error! cannot open [%s] for writing: %s\n", liftn.c_str(), strerror(errno)); }
	FILE *reg_fp = NULL;
	if (want_regions && !(reg_fp = fopen(regn.c_str(), "w"))) { out_failed = true; fprintf(stderr, "Error! cannot open [%s] for writing: %s\n", regn.c_str(), strerror(errno)); }
	FILE *track_fp = NULL, *qtrack_fp = NULL;
	if (qtrack_w && !(qtrack_fp = fopen(qtrackn.c_str(), "w"))) { out_failed = true; fprintf(stderr, "Error! cannot open [%s] for writing: %s\n", qtrackn.c_str(), strerror(errno)); }
	if (track_w && !(track_fp = fopen(trackn.c_str(), "w"))) { out_failed = true; fprintf(stderr, "Error! cannot open [%s] for writing: %s\n", trackn.c_str(), strerror(errno)); }
	FILE *chain_fp = NULL; int64_t chain_id = 0;
	if (want_chain && !(chain_fp = fopen(chainn.c_str(), "w"))) { out_failed = true; fprintf(stderr, "Error! cannot open [%s] for writing: %s\n", chainn.c_str(), strerror(errno)); }
	FILE *proj_fp = NULL;
	if (want_proj && !(proj_fp = fopen(projn.c_str(), "w"))) { out_failed = true; fprintf(stderr, "Error! cannot open [%s] for writing: %s\n", projn.c_str(), strerror(errno)); }
	auto write_contig = [&](size_t ci, ContigResult &cr) {
		fprintf(stderr, "\tProcess query chromsomoe: %s...\n", qs[ci].name.c_str());
		if (chain_fp) {      // (in front of the emitters that shorten a block's last record: the chain reads the trim off the untrimmed one and changes nothing; never the host comparator in place of a missing device answer)
			if (sink.gblk[ci].size() != cr.blocks.size()) { if (!cr.blocks.empty()) { out_failed = true; fprintf(stderr, "Error! %d blocks, chain segments of %d\n", (int)cr.blocks.size(), (int)sink.gblk[ci].size()); } }
			else if (!cr.blocks.empty()) em.chain_text(qs[ci], cr, sink.gblk[ci].data(), sink.gseg[ci].data(), &chain_id, [&](OutBuf &&o) { if (o.n && fwrite(o.p, 1, o.n, chain_fp) != o.n) out_failed = true; });
			sink.gblk[ci].reset(); sink.gseg[ci].reset();
		}
		if (qtrack_fp) {      // (query contigs in file order, a contig's windows ascending; a contig without alignments has none)
			em.qtrack_text(ci == 0, qs[ci], sink.qtrack[ci].data(), (int64_t)sink.qtrack[ci].size(), [&](OutBuf &&o) { if (o.n && fwrite(o.p, 1, o.n, qtrack_fp) != o.n) out_failed = true; });
			sink.qtrack[ci].reset();
		}
		if (track_fp) {      // (query contigs in file order, a contig's windows ascending; a contig without alignments has none)
			em.track_text(ci == 0, qs[ci], sink.track[ci].data(), (int64_t)sink.track[ci].size(), [&](OutBuf &&o) { if (o.n && fwrite(o.p, 1, o.n, track_fp) != o.n) out_failed = true; });
			sink.track[ci].reset();
		}
		if (lift_fp) {      // (query contigs in file order, a contig's hits in input order; a contig without alignments has none)
			em.lift_text(ci == 0, qs[ci], cr, sink.lift[ci].data(), (int64_t)sink.lift[ci].size(), lift_chr.data(), lift_at.data(), [&](OutBuf &&o) { if (o.n && fwrite(o.p, 1, o.n, lift_fp) != o.n) out_failed = true; });
			sink.lift[ci].reset();
		}
		if (reg_fp) {      // (query contigs in file order, a contig's hits in input order; a contig without alignments has none)
			em.regions_text(ci == 0, qs[ci], cr, sink.regions[ci].data(), (int64_t)sink.regions[ci].size(), bed_chr.data(), bed_lo.data(), bed_hi.data(), bed_name.data(), [&](OutBuf &&o) { if (o.n && fwrite(o.p, 1, o.n, reg_fp) != o.n) out_failed = true; });
			sink.regions[ci].reset();
		}
		if (cr.blocks.empty()) return;
		long long len = 0, score = 0;
		for (size_t b = 0; b < cr.blocks.size(); b++) { len += cr.blocks[b].aln_len; score += cr.blocks[b].score; if (cr.blocks[b].bdup) n_dup++; }
		n_aln += (long long)cr.blocks.size(); tot_len += len; tot_match += score;
		fprintf(stderr, "\t\tProduce %d local alignments (length = %lld), ANI=%.2f%%\n", (int)cr.blocks.size(), len, 100 * (1.0 * score / len));
		if (fmt == 1 || fmt == 3) {      // (the PAF file is opened, queued and closed as the MAF file is)
			const double t = now_s();
			if (maf_fd < 0 || ci == 0) {
				if (maf_w) { if (!maf_w->close()) out_failed = true; maf_w.reset(); }
				if (maf_fd >= 0) close(maf_fd);
				maf_fd = open(maf.c_str(), O_WRONLY | O_CREAT | (ci == 0 ? O_TRUNC : O_APPEND), 0644);
				if (maf_fd >= 0) maf_w.reset(new OrderedWriter(maf_fd));
				else if (!out_failed) { out_failed = true; fprintf(stderr, "Error! cannot open [%s] for writing: %s\n", maf.c_str(), strerror(errno)); }
			}
			if (maf_w && fmt == 3 && sink.cblk[ci].size() != cr.blocks.size()) {      // (never the host comparator in place of a missing device answer)
				out_failed = true; fprintf(stderr, "Error! %d blocks, CIGARs of %d\n", (int)cr.blocks.size(), (int)sink.cblk[ci].size());
			} else if (maf_w && fmt == 3 && want_cs && sink.sblk[ci].size() != cr.blocks.size()) {
				out_failed = true; fprintf(stderr, "Error! %d blocks, cs strings of %d\n", (int)cr.blocks.size(), (int)sink.sblk[ci].size());
			} else if (maf_w && fmt == 3) em.paf_text(qs[ci], cr, sink.cblk[ci].data(), sink.cops[ci].data(), [&](OutBuf &&o) { maf_w->push(std::move(o)); },
			                                          want_cs ? sink.sblk[ci].data() : nullptr, want_cs ? sink.sbytes[ci].data() : nullptr);
			else if (maf_w) em.maf_text(ci == 0, qs[ci], cr, [&](OutBuf &&o) { maf_w->push(std::move(o)); }, [&](size_t c) { return maf_w->take(c); });
			sink.cblk[ci].reset(); sink.cops[ci].reset(); sink.sblk[ci].reset(); sink.sbytes[ci].reset();
			t_maf_fmt += now_s() - t;
		}
		if (fmt == 2) {
			FILE *fp = fopen(aln.c_str(), ci == 0 ? "w" : "a");
			if (fp) { em.aln(fp, qs[ci], cr); if (ferror(fp) | fclose(fp)) out_failed = true; }
			else if (!out_failed) { out_failed = true; fprintf(stderr, "Error! cannot open [%s] for writing: %s\n", aln.c_str(), strerror(errno)); }
		}
		if (vcf) {
			const double t = now_s();
			if (var_on_gpu) { em.variants_from((int)ci, qs[ci], sink.var[ci].data(), (int64_t)sink.var[ci].size()); sink.var[ci].reset(); }
			else em.variants((int)ci, qs[ci], cr);
			t_var += now_s() - t;
		}
		if (dotplot && !gnuplot.empty()) {                               // GSAlign.cpp:546: only when gnuplot was found (main.cpp:324)
			const std::string gp = std::string(out_prefix) + ".gp";
			std::vector<std::string> data_files;
			if (em.dotplot(gp, out_prefix, qs[ci], cr, &data_files)) {
				fprintf(stderr, "\t\tGenerate dotplot for query sequence (%s-%s.ps)\n", out_prefix, qs[ci].name.c_str());
				if (system((gnuplot + " " + gp).c_str()) != 0) fprintf(stderr, "\t\tgnuplot failed\n");
				// (the reference shells out to `rm <prefix>.<contig name>*` with the raw FASTA header name, DotPloting.cpp:70: the
				//  files it means are exactly the data files written above)
				for (const std::string &fn : data_files) (void)remove(fn.c_str());
			}
		}
	};
	std::thread formatter([&] {
		for (size_t k = 0; k < qs.size(); k++) {
			{ std::unique_lock<std::mutex> lk(sink.mu); sink.cv.wait(lk, [&] { return sink.abort || sink.ready[k]; }); if (!sink.ready[k]) return; }
			write_contig(k, sink.res[k]);
			ContigResult().blocks.swap(sink.res[k].blocks); sink.res[k].recs.reset();
			sink.res[k].aln1.reset(); sink.res[k].aln2.reset();
			written = k + 1;
		}
	});
	auto on_result = [](void *user, int32_t ci, const gsa_result *res) -> int {
		Sink &sk = *(Sink *)user;
		const double t = now_s();
		sk.res[(size_t)ci].assign(*res);
		const double dt = now_s() - t;
		{ std::lock_guard<std::mutex> lk(sk.mu); sk.ready[(size_t)ci] = 1; sk.copy_s += dt; }
		sk.cv.notify_all();
		return 0;
	};
	// -gpuvar: the worker runs the variant pass in front of the callback (gsa_align_many_variants); the records are copied like the result
	auto on_result_var = [](void *user, int32_t ci, const gsa_result *res, const gsa_variants *var) -> int {
		Sink &sk = *(Sink *)user;
		const double t = now_s();
		sk.res[(size_t)ci].assign(*res);
		sk.var[(size_t)ci].assign(var->v, (size_t)var->n);
		const double dt = now_s() - t;
		{ std::lock_guard<std::mutex> lk(sk.mu); sk.ready[(size_t)ci] = 1; sk.copy_s += dt; }
		sk.cv.notify_all();
		return 0;
	};
	// -fmt 3: the worker runs the CIGAR pass (and with -gpuvar the variant pass) in front of the callback (gsa_align_many_ex); their records are copied like the result
	auto on_result_ex = [](void *user, int32_t ci, const gsa_result *res, const gsa_extras *ex) -> int {
		Sink &sk = *(Sink *)user;
		const double t = now_s();
		sk.res[(size_t)ci].assign(*res);
		if (ex->var) sk.var[(size_t)ci].assign(ex->var->v, (size_t)ex->var->n);
		if (ex->cig && sk.want_cig) { sk.cblk[(size_t)ci].assign(ex->cig->blk, (size_t)ex->cig->n_blocks); sk.cops[(size_t)ci].assign(ex->cig->ops, (size_t)ex->cig->n_ops); }
		if (sk.want_cs) {
			gsa_cs cs;
			if (gsa_extras_cs(ex, &cs) != GSA_OK) return 1;
			sk.sblk[(size_t)ci].assign(cs.blk, (size_t)cs.n_blocks); sk.sbytes[(size_t)ci].assign(cs.cs, (size_t)cs.n_bytes);
		}
		if (sk.want_lift) {
			gsa_lifts lf;
			if (gsa_extras_lift(ex, &lf) != GSA_OK) return 1;
			sk.lift[(size_t)ci].assign(lf.hits, (size_t)lf.n_hits);
		}
		if (sk.want_regions) {
			gsa_region_lifts rg;
			if (gsa_extras_regions(ex, &rg) != GSA_OK) return 1;
			sk.regions[(size_t)ci].assign(rg.hits, (size_t)rg.n_hits);
		}
		if (sk.want_segs) {
			gsa_segs sg;
			if (gsa_extras_segs(ex, &sg) != GSA_OK) return 1;
			sk.gblk[(size_t)ci].assign(sg.blk, (size_t)sg.n_blocks); sk.gseg[(size_t)ci].assign(sg.seg, (size_t)sg.n_segs);
		}
		if (sk.want_qtrack) {
			gsa_qtracks qt;
			if (gsa_extras_qtrack(ex, &qt) != GSA_OK) return 1;
			sk.qtrack[(size_t)ci].assign(qt.win, (size_t)qt.n_win);
		}
		if (sk.want_track) {
			gsa_tracks tk;
			if (gsa_extras_track(ex, &tk) != GSA_OK) return 1;
			sk.track[(size_t)ci].assign(tk.win, (size_t)tk.n_win);
		}
		const double dt = now_s() - t;
		{ std::lock_guard<std::mutex> lk(sk.mu); sk.ready[(size_t)ci] = 1; sk.copy_s += dt; }
		sk.cv.notify_all();
		return 0;
	};
	if (timing && var_on_gpu) for (gsa_ctx *c : ctxs) (void)gsa_set_profiling(c, 8);      // (the variant passes' device time, for the GSA_VARIANT_PASS line)
	const double ta = now_s(); t_at_align = ta - T0;
	const int rc_many = (fmt == 3 || want_lift || track_w || qtrack_w || want_chain || want_proj || want_regions) ? gsa_align_many_ex(ctxs.data(), (int32_t)ctxs.size(), qptr.data(), qlen.data(), (int32_t)qs.size(), 0, (fmt == 3 ? GSA_WANT_CIGARS : 0u) | (want_cs ? GSA_WANT_CS : 0u) | (var_on_gpu ? GSA_WANT_VARIANTS : 0u) | (want_lift ? GSA_WANT_LIFT : 0u) | (track_w ? GSA_WANT_TRACK : 0u) | (want_chain ? GSA_WANT_SEGS : 0u) | (want_proj ? GSA_WANT_PROJ : 0u) | (want_regions ? GSA_WANT_REGIONS : 0u) | (qtrack_w ? GSA_WANT_QTRACK : 0u), on_result_ex, &sink)
	                  : var_on_gpu ? gsa_align_many_variants(ctxs.data(), (int32_t)ctxs.size(), qptr.data(), qlen.data(), (int32_t)qs.size(), 0, on_result_var, &sink)
	                               : gsa_align_many(ctxs.data(), (int32_t)ctxs.size(), qptr.data(), qlen.data(), (int32_t)qs.size(), 0, on_result, &sink);
	t_align = now_s() - ta;
	// where the contexts' host threads spent that time (gsa_get_wall_sums: [0] query set-up / wait for the upload, [s] stage s) and what growing buffers cost them
	if (timing && getenv("GSA_DUMP_BUFFERS")) for (gsa_ctx *c : ctxs) (void)gsa_debug_buffers(c, 24);
	double cigar_ms = 0;      // -fmt 3: wall time the workers spent inside gsa_block_cigars, all contexts
	double cs_ms = 0;         // -cs: the same of gsa_block_cs (which runs the CIGAR walk itself: cigar_s is 0 then)
	double lift_ms = 0;       // -lift: the same of gsa_lift
	double regions_ms = 0;    // -liftbed: the same of gsa_lift_regions
	double track_ms = 0;      // -track: the same of gsa_ref_track
	double qtrack_ms = 0;     // -qtrack: the same of gsa_query_track
	double chain_ms = 0;      // -chain: the same of gsa_block_segs (its CIGAR walk included unless -cs ran it)
	double proj_ms = 0;       // -proj: the same of gsa_project, plus the fetch, merge and write below
	double var_dev_ms = 0; long long var_dev_n = 0;      // -gpuvar: device time of the variant passes (hipEvents), all contexts
	double wall_sum[10] = { 0 }; double alloc_ms = 0; long long alloc_n = 0, alloc_bytes = 0;
	for (gsa_ctx *c : ctxs) {
		double w[10]; int64_t wn = 0; if (gsa_get_wall_sums(c, w, &wn) == GSA_OK) for (int k = 0; k < 9; k++) wall_sum[k] += w[k];
		{ double cm = 0; int64_t cn = 0; if (gsa_get_cigar_timing(c, &cm, &cn) == GSA_OK) cigar_ms += cm; }
		{ double cm = 0; int64_t cn = 0; if (gsa_get_cs_timing(c, &cm, &cn) == GSA_OK) cs_ms += cm; }
		{ double cm = 0; int64_t cn = 0; if (gsa_get_lift_timing(c, &cm, &cn) == GSA_OK) lift_ms += cm; }
		{ double cm = 0; int64_t cn = 0; if (gsa_get_region_timing(c, &cm, &cn) == GSA_OK) regions_ms += cm; }
		{ double cm = 0; int64_t cn = 0; if (gsa_get_track_timing(c, &cm, &cn) == GSA_OK) track_ms += cm; }
		{ double cm = 0; int64_t cn = 0; if (gsa_get_qtrack_timing(c, &cm, &cn) == GSA_OK) qtrack_ms += cm; }
		{ double cm = 0; int64_t cn = 0; if (gsa_get_seg_timing(c, &cm, &cn) == GSA_OK) chain_ms += cm; }
		{ double cm = 0; int64_t cn = 0; if (gsa_get_proj_timing(c, &cm, &cn) == GSA_OK) proj_ms += cm; }
		double vm = 0; int64_t vn = 0; if (gsa_get_variant_timing(c, &vm, &vn) == GSA_OK) { var_dev_ms += vm; var_dev_n += vn; }
		double am = 0; int64_t an = 0, ab = 0; if (gsa_get_alloc_stats(c, &am, &an, &ab) == GSA_OK) { alloc_ms += am; alloc_n += an; alloc_bytes += ab; }
	}
	// -proj: every contig is painted (gsa_align_many_ex has returned).  The words of every further GPU go into the first GPU's array, in chunks; the text comes home
	// sequence by sequence and is written as FASTA -- before the contexts are destroyed
	if (proj_fp && rc_many == GSA_OK) {
		const double t = now_s();
		bool ok = true;
		std::vector<uint32_t> wbuf;
		for (size_t g = 1; g < gpus.size() && ok; g++)
			for (int64_t p0 = 0; p0 < idx.G && ok; p0 += (int64_t)1 << 24) {
				const int64_t m = std::min<int64_t>((int64_t)1 << 24, idx.G - p0);
				wbuf.resize((size_t)m);
				if (gsa_proj_fetch(ctxs[g], p0, m, NULL, wbuf.data()) != GSA_OK) { fprintf(stderr, "-proj: %s\n", gsa_last_error(ctxs[g])); ok = false; }
				else if (gsa_proj_merge(ctxs[0], p0, m, wbuf.data()) != GSA_OK) { fprintf(stderr, "-proj: %s\n", gsa_last_error(ctxs[0])); ok = false; }
			}
		std::string text;
		for (size_t c = 0; c < idx.chr_len.size() && ok; c++) {
			text.resize((size_t)idx.chr_len[c]);
			if (gsa_proj_fetch(ctxs[0], idx.chr_fwd[c], idx.chr_len[c], &text[0], NULL) != GSA_OK) { fprintf(stderr, "-proj: %s\n", gsa_last_error(ctxs[0])); ok = false; break; }
			em.proj_text((int)c, text.data(), [&](OutBuf &&o) { if (o.n && fwrite(o.p, 1, o.n, proj_fp) != o.n) out_failed = true; });
		}
		if (!ok) out_failed = true;
		proj_ms += (now_s() - t) * 1e3;
	}
	if (proj_fp) { if (ferror(proj_fp) | fclose(proj_fp)) out_failed = true; proj_fp = NULL; }
	{ std::lock_guard<std::mutex> lk(sink.mu); if (rc_many != GSA_OK) sink.abort = true; }
	sink.cv.notify_all();
	const double td = now_s();
	// (the contexts are done with -- every result was copied by on_result: their teardown, 0.2 s of hipFree at human scale, runs beside the output's tail)
	double t_destroy = 0;
	std::thread destroyer([&] { if (rc_many != GSA_OK) return; const double t = now_s(); for (size_t k = ctxs.size(); k-- > 0;) gsa_destroy(ctxs[k]); t_destroy = now_s() - t; });      // clones before the owners of their index (after an error the contexts stay: their messages are printed below)
	formatter.join();
	if (lift_fp) { if (ferror(lift_fp) | fclose(lift_fp)) out_failed = true; lift_fp = NULL; }
	if (reg_fp) { if (ferror(reg_fp) | fclose(reg_fp)) out_failed = true; reg_fp = NULL; }
	if (track_fp) { if (ferror(track_fp) | fclose(track_fp)) out_failed = true; track_fp = NULL; }
	if (qtrack_fp) { if (ferror(qtrack_fp) | fclose(qtrack_fp)) out_failed = true; qtrack_fp = NULL; }
	if (chain_fp) { if (ferror(chain_fp) | fclose(chain_fp)) out_failed = true; chain_fp = NULL; }
	double maf_write_s = 0; unsigned long long maf_bytes = 0;
	// (the MAF writer still has its queue to write -- ~1 s at human scale: the VCF is sorted, formatted and written beside it, the MAF file is closed behind)
	auto close_maf = [&] {
		if (maf_w) { if (!maf_w->close()) out_failed = true; maf_write_s = maf_w->write_seconds(); maf_bytes = maf_w->bytes(); maf_w.reset(); }
		if (maf_fd >= 0) { if (close(maf_fd) != 0) out_failed = true; maf_fd = -1; }
	};
	t_copy = sink.copy_s;
	if (rc_many != GSA_OK) {
		close_maf(); destroyer.join();
		for (gsa_ctx *c : ctxs) if (*gsa_last_error(c)) fprintf(stderr, "GPU error: %s\n", gsa_last_error(c));
		fprintf(stderr, "\t%d of %d query sequences were written before the error\n", (int)written, (int)qs.size());
		return 2;
	}
	if (n_aln > 0) fprintf(stderr, "\tAlignment#=%d (total alignment length=%lld) ANI=%.2f%%, unique alignment#=%d\n", (int)n_aln, tot_len, 100 * (1.0 * tot_match / tot_len), (int)(n_aln - n_dup));
	fprintf(stderr, "\tIt took %lld seconds for genome sequence alignment.\n", (long long)(time(NULL) - t0));
	unsigned long long vcf_bytes = 0; double vcf_write_s = 0;
	if (vcf) {
		const double t = now_s();
		fprintf(stderr, "\nGSAlign identifies %d SNVs, %d insertions, and %d deletions [%s].\n\n", em.n_snv, em.n_ins, em.n_del, vcfn.c_str());
		const int fd = open(vcfn.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
		if (fd >= 0) {
			OrderedWriter w(fd);
			em.vcf_text(index_prefix != NULL ? index_prefix : ref_fa, [&](OutBuf &&o) { w.push(std::move(o)); });
			if (!w.close()) out_failed = true;
			vcf_bytes = w.bytes(); vcf_write_s = w.write_seconds();
			if (close(fd) != 0) out_failed = true;
		} else { out_failed = true; fprintf(stderr, "Error! cannot open [%s] for writing: %s\n", vcfn.c_str(), strerror(errno)); }
		t_vcf = now_s() - t;
	}
	close_maf();
	t_drain = now_s() - td;      // (from the last contig's alignment to both files closed; the VCF's time lies inside it now)
	destroyer.join();
	if (timing) {
		long long qbp = 0; for (const QueryContig &q : qs) qbp += (long long)q.seq.size();
		const double total = now_s() - T0;
		fprintf(stderr, "GSA_TIMING {\"total_s\": %.3f, \"index_build_s\": %.3f, \"index_load_s\": %.3f, \"gsa_create_s\": %.3f, \"query_load_s\": %.3f, \"query_pin_s\": %.3f, \"align_many_s\": %.3f, \"cigar_s\": %.3f, "
		        "\"result_copy_s_sum\": %.3f, \"maf_format_s\": %.3f, \"variants_s\": %.3f, \"output_drain_after_align_s\": %.3f, \"maf_write_s\": %.3f, \"maf_bytes\": %llu, "
		        "\"vcf_s\": %.3f, \"vcf_write_s\": %.3f, \"vcf_bytes\": %llu, \"destroy_s\": %.3f, \"host_threads\": %d, \"contexts\": %d, \"query_bp\": %lld, \"contigs\": %d, \"gbp_per_s_excl_index_build\": %.4f, "
		        "\"ref_unpack_s\": %.3f, \"reserve_s\": %.3f, \"reserve_wait_s\": %.3f, \"unpack_wait_s\": %.3f, \"align_starts_at_s\": %.3f, \"ctx_wall_ms_sum\": [%.1f, %.1f, %.1f, %.1f, %.1f, %.1f, %.1f, %.1f, %.1f], \"alloc_ms_sum\": %.1f, \"alloc_n\": %lld, \"alloc_gb\": %.2f, \"ref_parse_s\": %.3f, \"create_from_pac_s\": %.3f, \"qtrack_s\": %.3f, \"regions_s\": %.3f, \"proj_s\": %.3f, \"chain_s\": %.3f, \"track_s\": %.3f, \"lift_s\": %.3f, \"cs_s\": %.3f}\n",
		        total, t_build, t_index, t_create, t_query, t_pin, t_align, cigar_ms / 1e3, t_copy, t_maf_fmt, t_var, t_drain, maf_write_s, maf_bytes, t_vcf, vcf_write_s, vcf_bytes, t_destroy,
		        HostPool::global().threads(), (int)ctxs.size(), qbp, (int)qs.size(), (double)qbp / (total - t_build) / 1e9,
		        t_unpack, t_reserve, t_reserve_wait, t_unpack_wait, t_at_align, wall_sum[0], wall_sum[1], wall_sum[2], wall_sum[3], wall_sum[4], wall_sum[5], wall_sum[6], wall_sum[7], wall_sum[8], alloc_ms, alloc_n, (double)alloc_bytes / 1e9, t_ref_parse, t_from_pac, qtrack_ms / 1e3, regions_ms / 1e3, proj_ms / 1e3, chain_ms / 1e3, track_ms / 1e3, lift_ms / 1e3, cs_ms / 1e3);      // (cs_s stays the line's last field)
	}
	if (timing && var_on_gpu) fprintf(stderr, "GSA_VARIANT_PASS {\"device_ms_sum\": %.3f, \"passes\": %lld, \"query_bp\": %lld}\n", var_dev_ms, var_dev_n, [&] { long long b = 0; for (const QueryContig &q : qs) b += (long long)q.seq.size(); return b; }());
	// (everything is on disk and the GPU is released: the process ends here -- unwinding 20 GB of host buffers and the HIP runtime's own
	//  teardown cost a second or two of wall time at human scale and produce nothing)
	if (out_failed) fprintf(stderr, "Error! an output file could not be written completely (disk full?)\n");
	fflush(stdout); fflush(stderr);
	_exit(out_failed ? 1 : 0);
}
