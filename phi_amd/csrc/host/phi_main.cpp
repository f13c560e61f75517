// phi_main.cpp -- the `PHI` command-line driver: same flags, stderr log lines and FASTA output as
// the reference's src/main.cpp + the logging of ILP_index::ILP_function, with the hot path behind
// the C ABI of include/phi_amd.h (HIP kernels on one MI355X).  Own implementation.
//
//   ./PHI -g <target.gfa> -r <reads.fa> -o <haplotype.fasta> [-k -w -R -q -m -T -t -d -N -c]
//         [--device N | --devices 0,1,..] [--dp-budget RUNS]
//         [--coverage C0,C1,.. --genome-size N [--seed S]]   (-o 'out.{cov}x.fa': one FASTA per coverage)
//         [--keep-samples A,B,.. | --drop-samples A,B,.. | --panels N0,N1,.. [--panel-seed S] [--panel-always NAME,..]]
//         [--panel-auto N [--panel-blocks B] [--panel-always NAME,..]]   (the panel of N walks chosen from the reads)
//                                                             a panel of the graph's haplotypes, subset inside "set graph"
//                                                             (data/chop_graph.sh:46-66); -o 'out.{panel}.fa': one FASTA per panel
//         [--calls FILE [--calls-ref NAME] [--calls-contig NAME]]   the inferred haplotype as variant calls against a reference walk
//                                                             (plain-text VCF; one --calls per -o, in order, same placeholder)
//         [--calls-support]                                   FORMAT/AK and RK in every --calls file: the witness minimisers of ALT and REF, seen in the reads and all
//         [--bgzf]                                            every -o and --calls file as BGZF, compressed on the device
//         [--bgzf-index]                                      with --bgzf: FILE.tbi beside every --calls file, FILE.gzi and FILE.fai beside every -o file
//   ./PHI -g <target.gfa> -r a.fq -o a.fa -r b.fq -o b.fa ...      several read sets against ONE graph: the graph is parsed and
//         indexed once (the reference's harness runs PHI once per sample x coverage on the same graph,
//         data/run_batch_4_miqp.py:31-46), every job prints the log of a run of its own and writes its own FASTA
//
// -r reads.bam: a reads file is taken as BAM when it is gzip (BGZF or a single stream) and its inflated bytes begin with "BAM\1"
// -- by content, not by name; a gzip FASTA whose junk before the first header begins with these four bytes is therefore read
// as BAM.  The reads are the sequences `samtools fastq` would write with its default filter (records with flag & 0x900 left
// out, reverse-flagged records turned back), found and decoded on the device (phi_add_reads_bam); rules from
// the SAM/BAM specification, not compared with samtools.  Parking, several read sets, --coverage and --panels work as with
// FASTQ; one GPU only (refused with --devices of several).  CRAM and SAM text are refused.  One [M::main] BAM line states the counts.
//
// --devices: one context and one host thread per GPU; every GPU builds the full index, the chunks of the reads file are
// handed out in turn, the library's RCCL exchange (phi_comm_*) merges hit vectors and spectra once, and the first
// GPU solves and reports.  A read set smaller than --shard-min-bases per GPU uses fewer GPUs.
//
// Flag semantics (main.cpp:38-95): -q (IQP/ILP), -m (mixed/integer), -N (naive expanded graph)
// choose between formulations with the same optimum; they are accepted and mapped onto the one
// exact solver.  -t only sized OpenMP/Gurobi thread pools and is accepted and ignored.  The log
// lines scraped by the reference's evaluation scripts (data/postprocessing_2_MIQP.py:55-79) keep
// their exact formats.
//
// From process start to the closed FASTA what a small input pays is the HIP runtime, not the
// path: ~60-180 ms to start it, ~20 ms per hardware queue, and ~100 ms for the driver to take the process's GPU state
// down again when it ends.  So: the device context is made by a thread of its own while the graph is parsed; the reads
// file goes to the device as raw text (the records are found there: phi_add_reads_text); and the process that does
// the work can be a CHILD (PHI_DETACH=1) -- the parent returns the child's status the moment the FASTA is closed and the log
// written, the child's teardown (free of the arrays, the driver's cleanup: ~0.1 s at MHC size, ~1 s and 65 GB of HBM at
// chromosome scale) goes on behind it.  Off by default: when the reference's command returns its resources are free, and a
// harness that starts the next GPU job at once would find them still held.
// Exit status: 0; 1 on any error; 3 when --dp-budget was given and ran out before the path was proven optimal.
#include <errno.h>
#include <fcntl.h>
#include <stdarg.h>
#include <getopt.h>
#include <signal.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/prctl.h>
#include <sys/resource.h>
#include <sys/stat.h>
#include <sys/time.h>
#include <sys/wait.h>
#include <unistd.h>
#include <algorithm>
#include <atomic>
#include <functional>
#include <string>
#include <condition_variable>
#include <deque>
#include <future>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>
#include <zlib.h>
#include "../../../include/phi_amd.h"
#include "../../../include/phi_host.h"

#define PHI_VERSION "1.0-mi355x"

static double t0_real, cpu0;
static double realtime()
{
    struct timeval tp;
    gettimeofday(&tp, nullptr);
    return tp.tv_sec + tp.tv_usec * 1e-6;
}
static double cputime()
{
    struct rusage r;
    getrusage(RUSAGE_SELF, &r);
    return r.ru_utime.tv_sec + r.ru_stime.tv_sec + 1e-6 * (r.ru_utime.tv_usec + r.ru_stime.tv_usec) - cpu0;
}
static long peakrss()
{
    struct rusage r;
    getrusage(RUSAGE_SELF, &r);
    return r.ru_maxrss * 1024;
}
// "[M::func::<wall>*<cpu/wall>] " stamp of the reference (sys.cpp:92-117 users)
static void stamp(const char *func)
{
    const double w = realtime() - t0_real;
    fprintf(stderr, "[M::%s::%.3f*%.2f] ", func, w, cputime() / (w > 0 ? w : 1e-9));
}

// PHI_TIMING=1: the stages of the run, each with its begin and end on the process's clock (seconds since main was entered)
struct StageMarks {
    bool on = getenv("PHI_TIMING") != nullptr;
    std::mutex mu;
    struct M { std::string name; double b, e; };
    std::vector<M> marks;
    void add(const char *name, double b, double e)
    {
        if (!on) return;
        std::lock_guard<std::mutex> lk(mu);
        marks.push_back(M{name, b - t0_real, e - t0_real});
    }
    void clear() { std::lock_guard<std::mutex> lk(mu); marks.clear(); }
    void print()
    {
        if (!on) return;
        std::sort(marks.begin(), marks.end(), [](const M &a, const M &b) { return a.b < b.b; });
        fprintf(stderr, "[phi timing] main: entered at epoch %.6f\n", t0_real);
        for (const M &m : marks) fprintf(stderr, "[phi timing] main: stage %-34s %8.3f -> %8.3f s  (%9.3f ms)\n", m.name.c_str(), m.b, m.e, (m.e - m.b) * 1e3);
    }
};
static StageMarks g_marks;
struct Stage {
    const char *name; double b;
    explicit Stage(const char *n) : name(n), b(realtime()) {}
    ~Stage() { g_marks.add(name, b, realtime()); }
};

static void usage(FILE *fp, int k, int w, int R, int q, int m, float T, int t, const char *g, const char *r, const char *o, int d)
{
    fprintf(fp, "Usage: PHI -g <target.gfa> -r <reads.fa> -o <haplotype.fasta> \n");
    fprintf(fp, "Options:\n");
    fprintf(fp, "    -k INT       K-mer size [%d]\n", k);
    fprintf(fp, "    -w INT       Minimizer window size [%d]\n", w);
    fprintf(fp, "    -R INT       Recombination penalty [%d]\n", R);
    fprintf(fp, "    -q INT       Mode QP/ILP (default IQP i.e q1, use q0 for ILP) [%d]\n", q);
    fprintf(fp, "    -m INT       Mixed/Interger programming (default Mixed i.e -m1, use -m0 for Integer) [%d]\n", m);
    fprintf(fp, "    -T FLOAT     Threshold for minimizer filtering [%.3f]\n", T);
    fprintf(fp, "    -t INT       Threads [%d]\n", t);
    fprintf(fp, "    -g INT       GFA file [%s]\n", g);
    fprintf(fp, "    -r INT       Read [%s]\n", r);
    fprintf(fp, "    -o INT       Output haplotype [%s]\n", o);
    fprintf(fp, "    -d bool      Debug mode [%d]\n", d);
    fprintf(fp, "    --bgzf                 every -o and --calls file compressed into BGZF blocks on the GPU; names are taken as given\n");
    fprintf(fp, "    --bgzf-index           with --bgzf: a tabix index FILE.tbi of every --calls file and FILE.gzi + FILE.fai of every -o file, built with the file\n");
    fprintf(fp, "    --calls FILE           the inferred haplotype as variant calls (plain-text VCFv4.2; .gz only with --bgzf) against a reference walk of\n");
    fprintf(fp, "                           the graph; one per -o, in order, with the same {cov} / {panel} placeholder where -o takes one.\n");
    fprintf(fp, "                           The rule is this program's own (not vg deconstruct's): nothing is trimmed or left-aligned\n");
    fprintf(fp, "    --calls-support        with --calls: per record FORMAT/AK and RK, the minimisers that witness ALT and REF -- seen in the reads, all\n");
    fprintf(fp, "    --calls-ref NAME       the reference walk, named as the log names walks (SAMPLE.HAP); required with -g, REF.0 with --vcf;\n");
    fprintf(fp, "                           under a panel it must be among the kept walks (--panel-always keeps it)\n");
    fprintf(fp, "    --calls-contig NAME    the contig of the records [--vcf: the VCF's contig; -g: the reference walk's name].  With -g POS\n");
    fprintf(fp, "                           counts the walk's own bases from 1: a W-line's start offset is not kept by the reader\n");
    fprintf(fp, "    --region R             with --vcf and --ref: the graph of one region, R = NAME, NAME:BEG or NAME:BEG-END (1-based, inclusive, commas\n");
    fprintf(fp, "                           allowed, as tabix and samtools read it).  The VCF must be BGZF with its .tbi, the FASTA indexed (.fai; BGZF: .gzi);\n");
    fprintf(fp, "                           only the BGZF members the index points at are read.  --calls records stay in the contig's coordinates\n");
}

struct Options {
    int k = 31, w = 25, n_threads = 4, recombination = 100, is_qclp = 1, is_naive = 0, is_mixed = 1, debug = 0;
    int device = 0, max_occ = 5000;
    int chop = 0;                                             // --chop N: segments cut into pieces of at most N bases inside "set graph" (data/chop_graph.sh:3)
    std::vector<int> devices;                                 // --devices: one context (and host thread) per GPU
    long long dp_budget = -1;                                 // --dp-budget: DP runs of the exact search; not given: no limit, as model.optimize()
    long long shard_min_bases = 50000000;                     // --shard-min-bases: text bytes of reads a further GPU must be worth
    float threshold = 1.0f;
    std::string gfa_file, reads_file, hap_file;               // (reads_file / hap_file: the first job's, for the usage text)
    std::vector<int> reads_kinds;                             // per -r: its ReadsKind, decided once in main (from a regular file's first bytes)
    std::string vcf_ref;                                      // --vcf FILE --ref FILE: the graph from a phased VCF (gfa_file holds the VCF's name then)
    bool from_vcf = false;
    std::string region;                                       // --region R: one region of an indexed VCF and FASTA
    int vcf_max_len = 30;                                     // its segments' length (--chop N; gfa2gbwt -m 30, vcf2gfa.py:53)
    std::vector<std::string> reads_files, hap_files;          // one entry per job: -r a -o a.fa -r b -o b.fa ...
    // --coverage C0,C1,.. --genome-size N [--seed S]: every read set is inferred at a ladder of coverages (data/preprocess.py:83-107,
    // data/run_batch_4.py:38-58): collected once, sampled on the device, one FASTA per level (-o names them through {cov})
    std::vector<std::string> cov_names;                       // as written on the command line
    std::vector<double> cov;
    double genome_size = 0.0;
    unsigned long long seed = 0;
    // a panel of the graph's haplotypes (data/chop_graph.sh:46-66; the sample lists of data/get_ids.py, data/get_ids_2.py):
    // --keep-samples / --drop-samples A,B,.. or @FILE; --panels N0,N1,..: nested panels by sample (data/run_batch_9.py to run_batch_13.py)
    std::vector<std::string> keep_samples, drop_samples, panel_always;
    bool have_keep = false, have_drop = false;
    std::vector<std::string> panel_names;                     // the sizes as written on the command line
    std::vector<int> panel_sizes;
    unsigned long long panel_seed = 0;
    // --panel-auto N [--panel-blocks B]: the panel of N walks chosen from the reads, per read set (phi_scout_graph, phi_scout_scores,
    // phi_scout_choose: in the place of `vg haplotypes`, data/vg_haplotypes.py:21-29, in front of data/chop_graph.sh:46-66)
    int panel_auto = 0, panel_blocks = 0;
    // --calls FILE [--calls-ref NAME] [--calls-contig NAME]: the inferred path written as variant calls against a reference walk
    // (phi_calls_path, phi_write_calls_vcf; no reference counterpart: for the comparison of data/run_PG.py:54-60); one per -o
    std::vector<std::string> calls_files;
    std::string calls_ref, calls_contig;
    bool calls_support = false;                               // --calls-support: FORMAT/AK and RK in every --calls file (phi_calls_support)
    bool bgzf_index = false;                                  // --bgzf-index: the indexes of those files, built beside them
    bool bgzf = false;                                        // --bgzf: every -o and --calls file compressed into BGZF blocks on the device
    bool panel() const { return have_keep || have_drop || !panel_sizes.empty() || panel_auto > 0; }
    int argc = 0;
    char **argv = nullptr;
    bool detached = false;
};

// A,B,.. or @FILE (one name per line): the names of --keep-samples, --drop-samples, --panel-always
static bool read_names(const char *arg, std::vector<std::string> &out)
{
    out.clear();
    if (arg[0] == '@') {
        FILE *fp = fopen(arg + 1, "r");
        if (!fp) return false;
        char line[4096];
        while (fgets(line, sizeof line, fp)) {
            std::string t(line);
            while (!t.empty() && (t.back() == '\n' || t.back() == '\r' || t.back() == ' ' || t.back() == '\t')) t.pop_back();
            if (!t.empty()) out.push_back(t);
        }
        fclose(fp);
        return true;
    }
    std::string t;
    for (const char *p = arg;; p++) {
        if (*p == ',' || !*p) { if (!t.empty()) out.push_back(t); t.clear(); if (!*p) break; }
        else t.push_back(*p);
    }
    return true;
}
// output number ordinal + 1 of SplitMix64(seed): the key of phi_amd/panel.py nested_panels (phi_amd.ladder.splitmix64)
static uint64_t splitmix64(uint64_t seed, uint64_t ordinal)
{
    uint64_t x = seed + (ordinal + 1) * 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// ---- the PHI_* knobs of a run, read once
struct Knobs {
    static bool off(const char *name) { const char *e = getenv(name); return e && atoi(e) == 0; }      // set to 0
    static int64_t num(const char *name, int64_t dflt) { const char *e = getenv(name); return e ? atoll(e) : dflt; }
    bool allow_same_device = getenv("PHI_ALLOW_SAME_DEVICE") != nullptr;      // (the tests run two contexts on one GPU)
    bool read_chunk_set = getenv("PHI_READ_CHUNK") != nullptr;                // unset: the chunk is sized by the files (chunk_size)
    int64_t read_chunk = read_chunk_set ? std::max<int64_t>(256, num("PHI_READ_CHUNK", 0)) : ((int64_t)64 << 20);
    bool text_park = !off("PHI_TEXT_PARK");                                   // 0: neither the park nor the device inflater
    int64_t text_park_min = num("PHI_TEXT_PARK_MIN", (int64_t)256 << 20);
    int64_t text_park_max = num("PHI_TEXT_PARK_MAX", (int64_t)96 << 30);
    bool inflate = text_park && !off("PHI_INFLATE");
    int64_t inflate_min = num("PHI_INFLATE_MIN", (int64_t)16 << 20);
    bool gfa_inflate = !off("PHI_GFA_INFLATE");
    int64_t gfa_inflate_min = num("PHI_GFA_INFLATE_MIN", (int64_t)256 << 20);
    bool walks_host = getenv("PHI_WALKS") && !strcmp(getenv("PHI_WALKS"), "host");
    int64_t walk_text_min = num("PHI_WALK_TEXT_MIN", (int64_t)1 << 30);      // (see load_graph)
    bool exchange_peers = getenv("PHI_EXCHANGE") && !strcmp(getenv("PHI_EXCHANGE"), "peers");
    bool full_teardown = getenv("PHI_FULL_TEARDOWN") != nullptr;
};

// ---- what a file is: regular, its size, gzip (the 2-byte magic) and BGZF (a gzip header with the BC extra field)
struct FileProbe { bool regular = false; int64_t size = 0; bool gzip = false, bgzf = false; };
static FileProbe probe_file(const std::string &path)
{
    FileProbe p;
    struct stat st;
    if (stat(path.c_str(), &st) != 0 || !S_ISREG(st.st_mode)) return p;      // (nothing is read from a pipe)
    p.regular = true; p.size = (int64_t)st.st_size;
    if (FILE *fp = p.size > 0 ? fopen(path.c_str(), "rb") : nullptr) {
        unsigned char u[14];
        const size_t got = fread(u, 1, sizeof u, fp); fclose(fp);
        p.gzip = got >= 2 && u[0] == 0x1f && u[1] == 0x8b;
        p.bgzf = p.gzip && got == sizeof u && (u[3] & 4) && u[12] == 'B' && u[13] == 'C';
    }
    return p;
}
// ---- what a reads file holds, by CONTENT: BAM when it is gzip (BGZF or not) and its inflated bytes begin with "BAM\1" -- so a
// gzip FASTA whose junk before the first header begins with these four bytes is read as BAM --; CRAM by its magic and SAM text
// by a header line with its first field at its start (@HD\tVN:, @SQ\tSN:, @RG\tID:, @PG\tID:), both refused (only their names are known here); everything else is FASTA / FASTQ text.
enum ReadsKind { READS_TEXT, READS_BAM, READS_CRAM, READS_SAM };
// Only a REGULAR file is looked at, and with pread: nothing is ever consumed from a pipe, a FIFO or a process substitution
// (-r <(samtools fastq x.bam)), which are text for the reader to take as it always has.  Decided once per -r (Options::reads_kinds).
static ReadsKind reads_kind(const std::string &path)
{
    struct stat st;
    if (stat(path.c_str(), &st) != 0 || !S_ISREG(st.st_mode)) return READS_TEXT;      // (the reader reports what cannot be opened)
    const int fd = open(path.c_str(), O_RDONLY);
    if (fd < 0) return READS_TEXT;
    unsigned char u[8] = {0};
    const ssize_t got = pread(fd, u, 7, 0);
    close(fd);
    if (got >= 4 && !memcmp(u, "CRAM", 4)) return READS_CRAM;
    // SAM text: a header line with its first mandatory field (a FASTQ whose first read is merely NAMED HD, SQ, RG or PG stays text)
    if (got == 7 && (!memcmp(u, "@HD\tVN:", 7) || !memcmp(u, "@SQ\tSN:", 7) || !memcmp(u, "@RG\tID:", 7) || !memcmp(u, "@PG\tID:", 7))) return READS_SAM;
    if (got < 2 || u[0] != 0x1f || u[1] != 0x8b) return READS_TEXT;
    gzFile gz = gzopen(path.c_str(), "rb");
    if (!gz) return READS_TEXT;
    unsigned char m[4];
    const int n = gzread(gz, m, 4);
    gzclose(gz);
    return n == 4 && !memcmp(m, "BAM\1", 4) ? READS_BAM : READS_TEXT;
}

// a single-stream gzip file (not BGZF: that is the host pool's) of at least `least` bytes: one of the device inflaters' inputs
static bool single_gzip(const FileProbe &p, int64_t least) { return p.regular && p.size >= std::max<int64_t>(least, 18) && p.gzip && !p.bgzf; }
static bool read_file(const std::string &path, int64_t size, std::vector<char> &out)
{
    FILE *fp = fopen(path.c_str(), "rb");
    if (!fp) return false;
    out.resize((size_t)size);
    const bool ok = fread(out.data(), 1, out.size(), fp) == out.size();
    fclose(fp);
    return ok;
}

// PHI_READ_CHUNK bytes per chunk; unset, 64 MB -- or for small plain files one chunk of the file's size (of the largest file, when
// there are several jobs).  A gzip file, BGZF included, keeps 64 MB.
static int64_t chunk_size(const Knobs &kn, const std::vector<std::string> &files)
{
    if (kn.read_chunk_set) return kn.read_chunk;
    int64_t need = 0;
    for (const std::string &rf : files) {
        const FileProbe p = probe_file(rf);
        int64_t want = kn.read_chunk;
        if (p.regular && p.size > 0 && !p.gzip) want = std::min<int64_t>(kn.read_chunk, (p.size + 4095) & ~(int64_t)4095);
        need = std::max(need, want);
    }
    return need;
}

// ---- the reads file as raw text chunks, from the reader thread to the device thread(s)
// The reads file is streamed as TEXT: a host thread fills chunk buffers with the file's (inflated) bytes while
// the main thread parses the graph and builds the index; every chunk then goes to phi_add_reads_text, which finds the records on
// the device -- chunk i + 1 crosses the link while chunk i is sketched, and no byte of a regular file is looked at by a host core.
// Host memory stays bounded: 2 + GPUs buffers.
struct Chunk { char *text = nullptr; int64_t n = 0; int32_t parked = -1; };      // parked >= 0: the bytes wait in device memory (phi_text_park_*), no host buffer
struct ReadsFeed {
    // set before the reader thread first starts
    const Knobs *kn = nullptr;
    int device = 0, n_buf = 0;                                // the GPU of the park and of the device inflater (one-GPU runs); 2 + GPUs
    int64_t chunk_bytes = 0;                                  //  buffers of chunk_bytes: one in flight per GPU, two with the reader
    bool inflate_on = false;                                  // single-stream gzip reads: inflated on the device
    // under mu
    std::mutex mu; std::condition_variable cv;
    std::deque<Chunk> buf;                                    // (a deque: entries for parked pieces are added -- by the reader thread only -- while others are in use)
    std::deque<int> q_free, q_full;                           // buffer indices; a full entry with n == 0 ends the stream
    bool stop = false;
    // atomics (cv is notified when they change)
    std::atomic<bool> gfa_parsed{false}, index_built{false};  // parking may begin / it ends
    std::atomic<bool> park_pinned{false};                     // the reader thread pinned the chunk buffers (the feed threads then do not)
    std::atomic<bool> pinned{true};                           // no buffer failed to register
    // the reader thread's; the others read them once it is joined -- but park, which a taker of a parked piece reads after the
    // queue's lock handed the piece over
    phi_text_park *park = nullptr;
    bool park_on = false;                                     // reads text parked in device memory until the index is built
    int64_t parked_bytes = 0;
    phi_inflate_info inflated{};                              // the device inflater's totals, over all read sets
    int fly_slot = -1, fly_idx = -1;                          // the buffer whose copy to the park is on its way, and its piece
    char err[512] = "";                                       // the reader's error (and the host reader's: host_reader)
    // the feed threads' (one GPU's turn at a time: under turn_mu; of one read set)
    std::mutex turn_mu;
    std::vector<char> carry;                                  // several GPUs: the bytes the last turn left unfinished
    bool stream_done = false;
    int64_t stream_fed = 0;                                   // bytes of the stream taken from the queue so far
    int64_t host_bases = 0;                                   // bases through the host reader
    std::atomic<int> n_chunks{0};
    std::once_flag pin_once;                                  // (over all read sets)
    bool registered = false;                                  // under pin_once
    std::future<int> reader;                                  // (last: joined before the rest goes)

    bool alloc(const Knobs *knobs, int dev, int64_t bytes, int n, bool park_text, bool inflate)
    {
        kn = knobs; device = dev; chunk_bytes = bytes; n_buf = n; park_on = park_text; inflate_on = inflate;
        buf.resize((size_t)n_buf);
        for (auto &b : buf) if (!(b.text = (char *)malloc((size_t)chunk_bytes))) return false;
        return true;
    }
    void start(const std::string &rf)                         // a read set: every buffer free, nothing queued, the reader thread on it
    {
        {
            std::lock_guard<std::mutex> lk(mu);
            q_free.clear(); q_full.clear(); stop = false;
            for (int i = 0; i < n_buf; i++) { buf[(size_t)i].n = 0; q_free.push_back(i); }
        }
        err[0] = 0;
        carry.clear(); stream_done = false; stream_fed = host_bases = 0; n_chunks = 0;
        reader = std::async(std::launch::async, [this, rf]() { return read_all(rf); });
    }
    void stop_reader() { { std::lock_guard<std::mutex> lk(mu); stop = true; } cv.notify_all(); if (reader.valid()) reader.wait(); }
    void mark(std::atomic<bool> &stage) { stage = true; cv.notify_all(); }
    int take_full()                                           // blocks; the end marker stays in the queue for the other takers
    {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return !q_full.empty(); });
        const int s = q_full.front();
        if (buf[(size_t)s].n > 0) q_full.pop_front();
        return s;
    }
    Chunk *at(int s) { std::lock_guard<std::mutex> lk(mu); return &buf[(size_t)s]; }      // (entries never move; the deque's index may, while one is added)
    void give_free(int s) { { std::lock_guard<std::mutex> lk(mu); if (buf[(size_t)s].text) q_free.push_back(s); } cv.notify_all(); }
    void give_full(int s) { { std::lock_guard<std::mutex> lk(mu); q_full.push_back(s); } cv.notify_all(); }
    // (the reader thread: the only one that adds entries) a parked piece to the queue / the copy on its way has landed: its buffer is free
    void queue_parked(int64_t n, int32_t idx) { { std::lock_guard<std::mutex> lk(mu); buf.push_back(Chunk{nullptr, n, idx}); q_full.push_back((int)buf.size() - 1); } cv.notify_all(); }
    void land_in_flight() { if (fly_slot >= 0) { (void)phi_text_park_wait(park, fly_idx); give_free(fly_slot); fly_slot = -1; } }
    // a file of more than one chunk: the buffers are pinned, so that the device copy of every further chunk is a direct DMA
    // (pinning takes milliseconds: not worth it for a single chunk)
    void pin_buffers(phi_ctx *cx)
    {
        std::call_once(pin_once, [&]() {
            if (park_pinned.load()) return;                   // (the reader thread pinned them when it began to park chunks)
            registered = true;
            std::lock_guard<std::mutex> lk(mu);               // (the reader thread may be adding an entry for a parked chunk)
            for (auto &b : buf) if (b.text && phi_host_register(cx, b.text, (size_t)chunk_bytes) != PHI_OK) pinned = false;
        });
    }
    void teardown(phi_ctx *cx)                                // (the reader thread stopped)
    {
        if (park) phi_text_park_destroy(park);                // (unpins the chunk buffers it pinned)
        for (auto &cb : buf) { if (registered && cb.text) (void)phi_host_unregister(cx, cb.text); free(cb.text); }
    }
    // Single-stream gzip reads (not BGZF) of a one-GPU run, from PHI_INFLATE_MIN compressed bytes on: inflated on the device
    // (phi_text_park_gzip_*) instead of one host thread, the text parked in pieces of chunk_bytes that the
    // reads stage takes as it takes any parked chunk.  PHI_INFLATE=0 or PHI_TEXT_PARK=0 keeps the host inflater; a stream the
    // device finds corrupt goes to the host inflater too, which reports it as it always has.
    bool inflate_on_device(const std::string &rf)
    {
        if (!inflate_on) return false;
        const FileProbe p = probe_file(rf);
        std::vector<char> gz;
        if (!single_gzip(p, kn->inflate_min) || !read_file(rf, p.size, gz)) return false;      // (not gzip, or BGZF: nothing read)
        std::unique_lock<std::mutex> lk(mu);                  // the device is free once the GFA is parsed (as for parking)
        cv.wait(lk, [&] { return gfa_parsed.load() || index_built.load() || stop; });
        if (stop) return false;
        lk.unlock();
        if (!park && phi_text_park_create(device, &park) != PHI_OK) return false;
        int32_t first = -1, count = 0;
        phi_inflate_info info;
        if (phi_text_park_gzip_begin(park, chunk_bytes) != PHI_OK || phi_text_park_gzip_add(park, gz.data(), (int64_t)gz.size()) != PHI_OK ||
            phi_text_park_gzip_end(park, &first, &count, &info) != PHI_OK)
            return false;
        for (int32_t i = 0; i < count; i++) queue_parked(phi_text_park_bytes(park, first + i), first + i);
        inflated.out_bytes += info.out_bytes; inflated.in_bytes += info.in_bytes; inflated.chunks += info.chunks;
        inflated.confirmed += info.confirmed; inflated.redecoded += info.redecoded;
        return true;
    }
    // the chunk in `slot` to device memory (its buffer is the copy engine's until the copy has landed: the next chunk is read
    // into another one meanwhile, and the buffer of the copy before -- done by now -- goes back to the free ones)
    bool park_chunk(int slot, int64_t n)
    {
        bool ok = true;
        if (!park) {
            ok = phi_text_park_create(device, &park) == PHI_OK;
            for (auto &b : buf) if (ok && b.text && phi_text_park_pin(park, b.text, (size_t)chunk_bytes) != PHI_OK) ok = false;
            if (ok) park_pinned = true;
        }
        int32_t idx = -1;
        if (!ok || phi_text_park_add_async(park, buf[(size_t)slot].text, n, &idx) != PHI_OK) return false;
        parked_bytes += n;
        queue_parked(n, idx);
        land_in_flight();
        fly_slot = slot; fly_idx = idx;
        return true;
    }
    // the reader thread: the file's text into the queue, ended by an entry of n == 0 (n < 0: the reader failed)
    int read_all(const std::string &rf)
    {
        Stage st("reads file -> text chunks [thread]");
        phi_text_stream *ts = nullptr;
        const bool on_device = inflate_on_device(rf);         // (then only the end of the stream is left to queue)
        int r = on_device ? PHI_HOST_OK : phi_text_stream_open(rf.c_str(), &ts, err, sizeof err);
        int slot = -1;
        for (;;) {
            if (slot < 0) {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return !q_free.empty() || stop; });
                if (stop) break;
                slot = q_free.front(); q_free.pop_front();
            }
            int64_t n = r != PHI_HOST_OK ? r : on_device ? 0 : phi_text_stream_read(ts, buf[(size_t)slot].text, chunk_bytes, err, sizeof err);
            if (n < 0) r = (int)n;
            // While the graph is still being read and indexed the link and the HBM are idle: the chunk goes to device memory
            // now (phi_text_park_*), the host buffer is free for the next one at once, and when the index is there the reads
            // stage finds the text where the records are found anyway.  (One GPU; large files; until the index is built.)
            if (n > 0 && park_on && !index_built.load() && !gfa_parsed.load()) {
                // the GFA is still being read (all host threads, all of the memory bandwidth): chunks stay in their host buffers
                // as long as two more are free (parking needs two: one is read into while the other's copy is on its way); with
                // fewer, wait with this chunk in hand for the GFA or for a taker
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return gfa_parsed.load() || index_built.load() || q_free.size() >= 2 || stop; });
            }
            if (n > 0 && park_on && gfa_parsed.load() && !index_built.load() && parked_bytes + n <= kn->text_park_max) {
                if (park_chunk(slot, n)) { slot = -1; continue; }
                park_on = false;                              // no room or no device yet: the usual way from here on
            }
            land_in_flight();
            buf[(size_t)slot].n = n;                          // 0 ends the stream, a negative value ends it as failed
            give_full(slot);
            slot = -1;
            if (n <= 0) break;
        }
        land_in_flight();
        if (ts) phi_text_stream_close(ts);
        return r;
    }
    // the rest of the stream for the host reader: blocks straight from the queue (phi_reads_stream_open_blocks)
    struct QueueBlocks { ReadsFeed *f; int held = -1; std::vector<char> fetched; };
    static int64_t next_block_from_queue(void *user, const char **block)
    {
        QueueBlocks *qb = (QueueBlocks *)user;
        if (qb->held >= 0) { qb->f->give_free(qb->held); qb->held = -1; }
        const int s = qb->f->take_full();
        const Chunk &c = *qb->f->at(s);
        if (c.n <= 0) return c.n;                             // 0: the end; negative: the reader thread failed
        if (c.parked < 0) { qb->held = s; *block = c.text; return c.n; }
        // a piece that went to device memory before the graph was there: its bytes come back for the host reader
        qb->fetched.resize((size_t)c.n);
        if (phi_text_park_fetch(qb->f->park, c.parked, qb->fetched.data(), c.n) != PHI_OK) return -1;
        (void)phi_text_park_release(qb->f->park, c.parked);
        *block = qb->fetched.data();
        return c.n;
    }
    // the host reader over `prefix` + (rest_of_queue) the rest of the queue -> phi_add_reads on cx (under turn_mu)
    int host_reader(phi_ctx *cx, const char *prefix, int64_t n_prefix, bool rest_of_queue, int64_t stream_offset)
    {
        Stage st("host reader (kseq state machine)");
        QueueBlocks qb{this, -1, {}};
        phi_reads_stream *rs = nullptr;
        if (phi_reads_stream_open_blocks(prefix, n_prefix, rest_of_queue ? next_block_from_queue : nullptr, &qb, stream_offset, &rs, err, sizeof err) != PHI_HOST_OK) return PHI_ERR_INVALID;
        const int64_t cap_b = std::max<int64_t>((int64_t)1 << 20, std::min<int64_t>(chunk_bytes, (int64_t)64 << 20)), cap_r = cap_b / 32 + 1024;
        std::vector<char> hb((size_t)cap_b);
        std::vector<int64_t> ho((size_t)cap_r + 1);
        int r = PHI_OK;
        for (;;) {
            const int64_t n = phi_reads_stream_next(rs, hb.data(), cap_b, ho.data(), cap_r, err, sizeof err);
            if (n < 0) { r = PHI_ERR_INVALID; break; }
            if (n == 0) break;
            host_bases += ho[(size_t)n];
            if ((r = phi_add_reads(cx, hb.data(), ho.data(), n))) break;
        }
        phi_reads_stream_close(rs);
        if (qb.held >= 0) give_free(qb.held);
        if (r == PHI_ERR_INVALID && err[0]) fprintf(stderr, "[E::main] %s\n", err);
        return r;
    }
};

// The walks of g, whose text is on the device (phi_walk_text_upload, phi_gfa_gzip_split), resolved there: PHI_OK (their offsets
// are g's unless *irregular), phi_walk_text_resolve's error, or WALK_NAMES when the names are not <prefix><number>.
static const int WALK_NAMES = 1;                              // (no phi_status is positive)
static int resolve_walks_on_device(phi_ctx *ctx, phi_graph *g, uint32_t *irregular)
{
    const char *prefix = nullptr; int32_t prefix_n = 0; const int32_t *num2id = nullptr; int64_t n_num = 0;
    *irregular = 0;
    if (phi_graph_name_index(g, &prefix, &prefix_n, &num2id, &n_num) != PHI_HOST_OK) return WALK_NAMES;
    std::vector<int64_t> woff((size_t)phi_graph_n_walks(g) + 1, 0);
    const int r = phi_walk_text_resolve(ctx, prefix, prefix_n, num2id, n_num, phi_graph_n_vtx(g), woff.data(), irregular);
    if (!r && !*irregular) phi_graph_set_walk_off(g, woff.data());
    return r;
}

// ---- one run: the contexts, the reads feed and the graph, shared by every job
struct Driver {
    const Options &o;
    const Knobs kn;
    const bool timing = g_marks.on;
    std::vector<int> devices;                                 // the GPUs used (n_dev), one context each
    int n_dev = 0;
    std::vector<phi_ctx *> ctxs;
    std::shared_future<int> f_ctx;                            // made by threads of their own (joined before ctxs goes)
    phi_ctx *ctx = nullptr;                                   // the context that solves and reports
    ReadsFeed feed;
    phi_graph *g = nullptr;
    phi_vcf *vcf = nullptr;                                   // --vcf: the reader's handle (the unit tables build_index writes the walks from)
    int64_t region_contig_len = 0;                            // --region: the contig's length by its .fai (the reference held is the region's)
    char err[512] = "";
    std::string reads_file, hap_file;                         // the job at hand, and the name in its FASTA
    int reads_kind_now = 0;                                   // the job's ReadsKind (Options::reads_kinds)
    char hap_name[4096];
    std::atomic<bool> failed{false};                          // a GPU failed in the phase at hand (run_on_all)
    bool use_peers = false;                                   // the exchange: peer-mapped memory or RCCL (comm_id)
    void *peer_group = nullptr;
    unsigned char comm_id[PHI_COMM_ID_BYTES];
    struct { int64_t bytes = 0; int rc = 0; bool sent = false; } wt;      // the walk text the deferred GFA reader sent to the device
    // ---- a panel of the graph's haplotypes (--keep-samples, --drop-samples, --panels): keep[h] per walk of g, and what the
    //      context's walks and vertices are in g's terms once the panel is set
    std::vector<uint8_t> keep;
    std::vector<int32_t> kept_walks;                          // panel walk -> walk of g
    std::vector<std::vector<std::string>> panels;             // --panels: the samples of every panel
    std::string hap_pattern;                                  // --panels: the job's -o with {panel} replaced
    bool walks_retained = false;                              // --panels: the full entries are on the device (PHI_PANEL_RETAIN)
    phi_panel_info panel_info{};
    long long full_entries = 0;                               // walk entries handed to the panel step
    // --panel-auto: the graph holds more walks than asked for (else the ordinary route); the scout has been set once (the
    // context has its parameters and retains the full entries); the walk offsets the scout and the panel are set with
    bool auto_on = false, auto_scouted = false;
    std::vector<int64_t> auto_walk_off;
    bool panel_on() const { return o.panel() && (o.panel_auto <= 0 || auto_on); }
    // --calls: the job, coverage and panel at hand (what the placeholders of the job's --calls name stand for)
    int job_now = 0;
    std::string cov_now, panel_now;
    explicit Driver(const Options &opt) : o(opt), devices(opt.devices), reads_file(opt.reads_files[0]), hap_file(opt.hap_files[0]), reads_kind_now(opt.reads_kinds.empty() ? 0 : opt.reads_kinds[0]) {}

    // the one error exit: the message, the reader thread stopped, status 1
    __attribute__((format(printf, 2, 3))) int fail(const char *fmt, ...)
    {
        va_list ap;
        va_start(ap, fmt); vfprintf(stderr, fmt, ap); va_end(ap);
        feed.stop_reader(); return 1;
    }
    int fail_on(phi_ctx *cx, const char *what, int code) { return fail("[E::main] %s: %s: %s\n", what, phi_strerror(code), phi_last_error(cx)); }
    int gfa_failed()
    {
        if (err[0] == 'E') return fail("%s\n", err);         // walk error text of ILP_index.cpp:105
        if (!err[0]) return fail("[E::main] failed to load the GFA file\n");
        return fail("[E::main] failed to load the GFA file\n[E::main] %s\n", err);
    }
    int name_job() { return phi_hap_name(o.gfa_file.c_str(), reads_file.c_str(), hap_name, sizeof hap_name) < 0 ? fail("[E::main] output name too long\n") : 0; }
    void loaded() { stamp("main"); fprintf(stderr, "Loaded graph from: %s\n", o.gfa_file.c_str()); }
    // One phase of the job on every GPU, each on its own host thread.  All threads of a phase are joined before the next
    // begins, and a collective (RCCL) is a phase of its own that is entered only when the phase before returned 0 on every
    // GPU: a rank that failed can then never leave the others waiting inside ncclCommInitRank / ncclAllReduce.
    int run_on_all(const char *what, const std::function<int(int, phi_ctx *)> &fn)
    {
        if (n_dev == 1) { const int r = fn(0, ctx); if (r) failed = true; return r ? fail_on(ctx, what, r) : 0; }
        std::vector<std::future<int>> fs;
        for (int i = 0; i < n_dev; i++) fs.push_back(std::async(std::launch::async, [&, i]() { const int r = fn(i, ctxs[(size_t)i]); if (r) failed = true; return r; }));
        int bad = -1, brc = 0;
        for (int i = 0; i < n_dev; i++) { const int r = fs[(size_t)i].get(); if (r && bad < 0) { bad = i; brc = r; } }
        if (bad >= 0) {
            if (brc == PHI_ERR_WALK) fprintf(stderr, "Error: %s\n", phi_last_error(ctxs[(size_t)bad]));
            return fail_on(ctxs[(size_t)bad], what, brc);
        }
        return 0;
    }
    // A single-stream gzip GFA (not BGZF) of a one-GPU run, from PHI_GFA_INFLATE_MIN compressed bytes on (default 256 MB):
    // inflated and split on the device (phi_gfa_gzip_split).  The walk fields stay in HBM whatever
    // PHI_WALK_TEXT_MIN says, and only the rest of the text -- S-lines, L-lines, W-line heads -- comes to the host reader.
    // Whatever that route does not finish (a corrupt stream, a refused split, walks counted differently, names not
    // <prefix><number>, a W-line among the S-lines, irregular walk text) is read again from the file, from scratch, by
    // load_graph: messages, exit status and output are those of PHI_GFA_INFLATE=0.  True when g was made here.
    bool gfa_on_device()
    {
        const FileProbe p = probe_file(o.gfa_file);
        std::vector<char> gz;
        if (!single_gzip(p, kn.gfa_inflate_min)) return false;
        if (Stage st("GFA gzip read (device context starting)"); !read_file(o.gfa_file, p.size, gz)) return false;
        Stage st("GFA on the device: inflate, split, parse, walks");
        const char *why = f_ctx.get() ? "no device context" : nullptr;
        char *host_text = nullptr; int64_t host_n = 0;
        phi_gfa_gzip_info gi; memset(&gi, 0, sizeof gi);
        int r = why ? 0 : phi_gfa_gzip_split(ctxs[0], gz.data(), (int64_t)gz.size(), 0, &host_text, &host_n, &gi);
        std::vector<char>().swap(gz);
        if (!why && r) why = r == PHI_ERR_INVALID ? "gzip stream corrupt" : r == PHI_ERR_UNSUPPORTED ? "split refused" : "device error";
        if (!why && phi_gfa_read_deferred_text(host_text, host_n, o.gfa_file.c_str(), &g, err, sizeof err) != PHI_HOST_OK) why = "host reader failed on the split text";
        if (!why && phi_graph_n_walks(g) != gi.n_walks) why = "walk count differs from the host reader's";
        if (!why) {
            uint32_t irregular = 0;
            r = resolve_walks_on_device(ctxs[0], g, &irregular);
            why = r == WALK_NAMES ? "names not <prefix><number>, or a W-line among the S-lines" : r ? "walks on the device failed" : irregular ? "irregular walk text" : nullptr;
        }
        if (why) {
            if (g) { phi_graph_free(g); g = nullptr; }
            if (!f_ctx.get()) (void)phi_walk_text_upload(ctxs[0], nullptr, 0);          // (lets the text on the device go)
            err[0] = 0;
        }
        phi_gfa_gzip_free(host_text);                        // (the reader borrowed it until the walks were resolved)
        if (timing && !why)
            fprintf(stderr, "[phi timing] main: GFA: %lld bytes inflated on the device from %lld gzip bytes (%lld chunks); %lld bytes to the host, %lld bytes of %d walks kept on the device\n",
                    (long long)gi.text_bytes, (long long)gi.inflate.in_bytes, (long long)gi.inflate.chunks, (long long)gi.host_bytes, (long long)gi.walk_bytes, gi.n_walks);
        else if (timing)
            fprintf(stderr, "[phi timing] main: GFA: not on the device (%s): the host reader from the file\n", why);
        return !why;
    }
    static void upload_walk_text(void *user, const phi_host_walk_text *walks, int32_t n)      // (the GFA reader's callback: once there is enough text)
    {
        Driver &d = *static_cast<Driver *>(user);
        for (int32_t i = 0; i < n; i++) d.wt.bytes += walks[i].n;
        if (d.wt.bytes < d.kn.walk_text_min || d.f_ctx.get()) return;      // (no device: main reports it)
        static_assert(sizeof(phi_host_walk_text) == sizeof(phi_walk_text), "the two libraries' walk text records");
        d.wt.rc = phi_walk_text_upload(d.ctxs[0], reinterpret_cast<const phi_walk_text *>(walks), n);
        d.wt.sent = d.wt.rc == 0;
    }
    // ---- graph from a phased VCF + reference FASTA (vcf2gfa.py:27-64): the host reads the fixed columns, the
    //      device parses the genotype text, the host builds the per-vertex arrays; the walk entries are written on every GPU
    //      by build_index.  No GFA is written or read.
    int load_graph_vcf()
    {
        int r;
        if (!o.region.empty()) {
            // --region: the host plans which BGZF members the .tbi points at and slices the FASTA; the device inflates those
            // members and keeps exactly the region's records; the rule pass then runs over header + kept lines
            phi_region *rg = nullptr;
            {
                Stage st("VCF region plan (host: .tbi, .fai, members)");
                r = phi_region_open(o.gfa_file.c_str(), o.vcf_ref.c_str(), o.region.c_str(), &rg, err, sizeof err);
            }
            if (r != PHI_HOST_OK) return fail("[E::region] %s\n", err);
            char *lines = nullptr;
            int64_t n_lines = 0;
            phi_vcf_region_info ri;
            int frc;
            {
                Stage st("VCF region filter (device: inflate + records)");
                frc = phi_vcf_region_filter(o.device, phi_region_gz(rg), phi_region_n_gz(rg), phi_region_ranges(rg), phi_region_n_ranges(rg), phi_region_name(rg),
                                            phi_region_beg(rg), phi_region_end(rg), &lines, &n_lines, &ri);
            }
            if (frc) { phi_region_free(rg); return fail("[E::region] %s\n", ri.detail); }
            fprintf(stderr, "Region %s:%lld-%lld of %lld bases: %lld BGZF members (%lld bytes, %lld inflated), %lld lines seen, %lld kept, %lld batch(es); GPU inflate %.3f ms, filter %.3f ms\n",
                    phi_region_name(rg), (long long)phi_region_beg(rg) + 1, (long long)phi_region_end(rg), (long long)phi_region_contig_len(rg), (long long)ri.members,
                    (long long)ri.gz_bytes, (long long)ri.text_bytes, (long long)ri.lines_seen, (long long)ri.lines_kept, (long long)ri.batches, ri.inflate_ms, ri.filter_ms);
            region_contig_len = phi_region_contig_len(rg);
            {
                Stage st("VCF + FASTA read (region)");
                r = phi_vcf_read_region(rg, lines, n_lines, &vcf, err, sizeof err);
            }
            phi_vcf_region_free(lines);
            phi_region_free(rg);
        } else {
            Stage st("VCF + FASTA read");
            r = phi_vcf_read(o.gfa_file.c_str(), o.vcf_ref.c_str(), &vcf, err, sizeof err);
        }
        if (r != PHI_HOST_OK) return fail("[E::vcf2gfa] %s\n", err);
        if (const long long n = phi_vcf_n_outside(vcf); n && !o.region.empty())
            fprintf(stderr, "[W::region] %lld record(s) skipped: they reach over an edge of the region %s\n", n, o.region.c_str());
        if (const long long n = phi_vcf_n_other_contig(vcf))
            fprintf(stderr, "[W::vcf2gfa] %lld record(s) of other contigs than %s skipped (vcf2gfa handles one contig)\n", n, phi_vcf_contig(vcf));
        if (const long long n = phi_vcf_n_ref_mismatch(vcf))
            fprintf(stderr, "[W::vcf2gfa] %lld record(s) skipped: their REF column is not what the FASTA holds at POS (another assembly?)\n", n);
        const int64_t n_rec = phi_vcf_n_records(vcf);
        const int32_t n_s = phi_vcf_n_samples(vcf);
        std::vector<uint16_t> gt((size_t)n_rec * (size_t)n_s * 2 + 1, 0);
        std::vector<int32_t> ploidy((size_t)n_s + 1, 0);
        std::vector<uint8_t> flagged((size_t)n_rec + 1, 0);
        {
            Stage st("VCF genotypes on the device");
            if ((r = f_ctx.get())) return fail("[E::main] no usable MI355X (HIP) device %d: %s\n", devices[0], phi_strerror(r));
            r = phi_vcf_genotypes(ctxs[0], phi_vcf_text(vcf), phi_vcf_text_off(vcf)[n_rec], phi_vcf_text_off(vcf), phi_vcf_rec_gt_index(vcf), n_rec, n_s,
                                  gt.data(), ploidy.data(), flagged.data());
            if (r) return fail_on(ctxs[0], "VCF genotypes", r);
            for (int64_t i = 0; i < n_rec; i++)                // what the kernel left undecided: the exact scalar parser
                if (flagged[(size_t)i] && phi_vcf_parse_gt(phi_vcf_text(vcf), phi_vcf_text_off(vcf), phi_vcf_rec_gt_index(vcf), i, i + 1, n_s, gt.data(), ploidy.data(), err, sizeof err))
                    return fail("[E::vcf2gfa] %s\n", err);
        }
        Stage st("VCF graph build");
        if (phi_vcf_build(vcf, gt.data(), ploidy.data(), o.vcf_max_len, &g, err, sizeof err) != PHI_HOST_OK) return fail("[E::vcf2gfa] %s\n", err);
        feed.mark(feed.gfa_parsed);
        return 0;
    }
    // ---- graph (main.cpp:101-115)
    // One GPU: the walks stay TEXT in the reader (include/phi_host.h phi_gfa_read_deferred) and go to HBM as soon as the reader
    // knows where they are -- while it still enters the segment names --, and the device resolves them (phi_walk_text_*): at
    // chromosome scale the walks are 96% of the file.  Text the device path does not take (reverse steps, names of another form:
    // walk_text.hip) is resolved by the host after all, with the reference's rules.  Small files (PHI_WALK_TEXT_MIN bytes of
    // walk text, default 1 GB) and multi-GPU runs (every GPU needs the walks) stay with the host.  (1 GB: the host threads resolve
    // 70 MB of walk text -- a 49-walk MHC graph -- in 10 ms, hidden behind the 0.1 s the HIP runtime takes to start, while the device
    // path has to wait for that start before its first byte moves: measured at C2, 32 MB as the threshold cost every process 40 ms)
    int load_graph()
    {
        if (o.from_vcf) return load_graph_vcf();
        const bool defer_walks = n_dev == 1 && !kn.walks_host;
        const bool on_device = defer_walks && kn.gfa_inflate && gfa_on_device();
        if (!on_device) {
            Stage st("GFA read + parse");
            const int r = defer_walks ? phi_gfa_read_deferred(o.gfa_file.c_str(), &g, upload_walk_text, this, err, sizeof err)
                                      : phi_gfa_read(o.gfa_file.c_str(), &g, err, sizeof err);
            if (r != PHI_HOST_OK) return gfa_failed();
        }
        feed.mark(feed.gfa_parsed);                           // (the reads text may go to device memory from here on)
        if (!defer_walks || on_device) return 0;
        Stage st("walks");
        bool walks_on_device = false;
        if (wt.rc) return fail("[E::main] walk text to the device: %s: %s\n", phi_strerror(wt.rc), phi_last_error(ctxs[0]));
        if (wt.sent) {
            uint32_t irregular = 0;
            const int r = resolve_walks_on_device(ctxs[0], g, &irregular);
            if (r == WALK_NAMES) (void)phi_walk_text_upload(ctxs[0], nullptr, 0);      // (lets the text on the device go)
            else if (r) return fail("[E::main] walks on the device: %s: %s\n", phi_strerror(r), phi_last_error(ctxs[0]));
            walks_on_device = r == PHI_OK && !irregular;
            if (timing) fprintf(stderr, "[phi] walks: %lld bytes of text %s\n", (long long)wt.bytes, walks_on_device ? "resolved on the device" : irregular ? "irregular for the device: host" : "names not <prefix><number>: host");
        }
        if (!walks_on_device && phi_graph_resolve_walks(g, err, sizeof err) != PHI_HOST_OK) return gfa_failed();
        return 0;
    }
    // ---- the panel: samples are the W-lines' sample fields (the VCF's sample names, REF for the reference walk)
    static std::string sample_of(const char *hap_name)
    {
        const char *dot = strrchr(hap_name, '.');
        return dot ? std::string(hap_name, dot) : std::string(hap_name);
    }
    std::vector<std::string> samples_in_order() const
    {
        std::vector<std::string> out;
        for (int32_t h = 0; h < phi_graph_n_walks(g); h++) {
            const std::string sm = sample_of(phi_graph_hap_name(g, h));
            if (std::find(out.begin(), out.end(), sm) == out.end()) out.push_back(sm);
        }
        return out;
    }
    int check_names(const char *option, const std::vector<std::string> &names, const std::vector<std::string> &have)
    {
        std::string missing;
        for (const std::string &n : names)
            if (std::find(have.begin(), have.end(), n) == have.end()) missing += (missing.empty() ? "" : ", ") + n;
        return missing.empty() ? 0 : fail("[E::main] %s: the graph holds no sample named %s\n", option, missing.c_str());
    }
    // keep[] from a list of samples to keep, or to drop
    void mask_of(const std::vector<std::string> &names, bool drop)
    {
        const int32_t n_walks = phi_graph_n_walks(g);
        keep.assign((size_t)n_walks, 0);
        for (int32_t h = 0; h < n_walks; h++) {
            const bool in = std::find(names.begin(), names.end(), sample_of(phi_graph_hap_name(g, h))) != names.end();
            keep[(size_t)h] = in != drop;
        }
    }
    // the options checked against the graph's samples; --panels: the nested panels of phi_amd/panel.py nested_panels
    int plan_panels()
    {
        if (!o.panel()) return 0;
        const std::vector<std::string> have = samples_in_order();
        if (o.panel_auto > 0) {
            if (!o.panel_always.empty() && check_names("--panel-always", o.panel_always, have)) return 1;
            auto_on = phi_graph_n_walks(g) > o.panel_auto;
            if (!auto_on) fprintf(stderr, "[M::main] --panel-auto %d: the graph holds %d walks, no more than asked for: the ordinary route, every walk kept\n", o.panel_auto, phi_graph_n_walks(g));
            return 0;
        }
        if (o.have_keep) { if (check_names("--keep-samples", o.keep_samples, have)) return 1; mask_of(o.keep_samples, false); return 0; }
        if (o.have_drop) { if (check_names("--drop-samples", o.drop_samples, have)) return 1; mask_of(o.drop_samples, true); return 0; }
        if (check_names("--panel-always", o.panel_always, have)) return 1;
        std::vector<std::string> rest;
        for (const std::string &sm : have)
            if (std::find(o.panel_always.begin(), o.panel_always.end(), sm) == o.panel_always.end()) rest.push_back(sm);
        if (o.panel_sizes.back() > (int)rest.size())
            return fail("[E::main] --panels: a panel of %d samples, but the graph holds %zu besides the always-kept ones\n", o.panel_sizes.back(), rest.size());
        std::vector<size_t> order(rest.size());
        for (size_t i = 0; i < order.size(); i++) order[i] = i;
        std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return splitmix64(o.panel_seed, a) < splitmix64(o.panel_seed, b); });
        for (int n : o.panel_sizes) {
            std::vector<std::string> p(o.panel_always);
            for (int i = 0; i < n; i++) p.push_back(rest[order[(size_t)i]]);
            panels.push_back(p);
        }
        return 0;
    }
    const char *walk_name(int32_t h) const { return phi_graph_hap_name(g, panel_on() ? kept_walks[(size_t)h] : h); }
    // "Panel: kept 13 of 49 walks (6 of 24 samples + REF): V -> V' vertices, E -> E' edges, X -> X' walk entries"
    void log_panel()
    {
        std::vector<std::string> all, in;
        bool ref_in = false;
        for (int32_t h = 0; h < phi_graph_n_walks(g); h++) {
            const std::string sm = sample_of(phi_graph_hap_name(g, h));
            const bool is_ref = sm == "REF";
            if (is_ref) { ref_in = ref_in || keep[(size_t)h]; continue; }
            if (std::find(all.begin(), all.end(), sm) == all.end()) all.push_back(sm);
            if (keep[(size_t)h] && std::find(in.begin(), in.end(), sm) == in.end()) in.push_back(sm);
        }
        const phi_panel_info &pi = panel_info;
        stamp("main");
        fprintf(stderr, "Panel: kept %d of %d walks (%zu of %zu samples%s): %lld -> %lld vertices, %lld -> %lld edges, %lld -> %lld walk entries\n",
                (int)kept_walks.size(), phi_graph_n_walks(g), in.size(), all.size(), ref_in ? " + REF" : "", (long long)phi_graph_n_vtx(g), (long long)pi.n_vtx_out,
                (long long)phi_graph_adj_off(g)[phi_graph_n_vtx(g)], (long long)pi.n_edges_out, (long long)full_entries, (long long)pi.n_entries_out);
    }
    // ---- --panel-auto, stage 1a: the index of EVERY walk without the DP (phi_scout_graph).  The first time from the graph's entries
    //      (the host's, those resolved on the device, or written there from the VCF's tables); for a further read set from the
    //      entries the context retained.
    int scout_index()
    {
        const uint32_t flags = (o.is_qclp ? PHI_FLAG_QCLP : 0) | (o.is_mixed ? PHI_FLAG_MIXED : 0);
        Stage st("phi_scout_graph (index of every walk)");
        const int32_t n_walks = phi_graph_n_walks(g);
        int r = auto_scouted ? 0 : phi_set_params(ctx, o.k, o.w, o.threshold, o.recombination, flags);
        if (!r) r = phi_set_solve_budget(ctx, o.dp_budget >= 0 ? o.dp_budget : 0);
        if (!r && !auto_scouted) {
            auto_walk_off.assign((size_t)n_walks + 1, 0);
            if (vcf) r = phi_vcf_walks_wide(ctx, phi_vcf_unit_first(vcf), phi_vcf_n_units(vcf), phi_vcf_site_backbone(vcf), phi_vcf_site_allele0(vcf),
                                            phi_vcf_n_real_sites(vcf), phi_vcf_choice(vcf), phi_vcf_n_kept_haps(vcf), auto_walk_off.data());
            else memcpy(auto_walk_off.data(), phi_graph_walk_off(g), auto_walk_off.size() * 8);
        }
        if (!r)
            r = phi_scout_graph(ctx, phi_graph_n_vtx(g), phi_graph_seq_concat(g), phi_graph_seq_off(g), phi_graph_adj_off(g), phi_graph_adj(g), n_walks,
                                auto_walk_off.data(), auto_scouted || vcf ? nullptr : phi_graph_walk_vtx(g), phi_graph_topo_rank(g));
        if (r == PHI_ERR_WALK) fprintf(stderr, "Error: %s\n", phi_last_error(ctx));
        if (r) { failed = true; return fail_on(ctx, "scout graph", r); }
        auto_scouted = true;
        full_entries = auto_walk_off[(size_t)n_walks];
        return 0;
    }
    // ---- --panel-auto, one read set: collected and scored against the scout, the panel chosen and set, the same reads scored
    //      against the panel's index, then solve and report as ever
    int run_auto_job()
    {
        int rc;
        const int32_t n_walks = phi_graph_n_walks(g);
        if ((rc = phi_reads_collect_begin(ctx, 0))) return fail_on(ctx, "collect", rc);
        if (Stage st("reads: text -> device, records (collected)"); run_on_all("reads", [&](int, phi_ctx *cx) -> int { return feed_reads(cx); })) return 1;
        if (feed.reader.get() != PHI_HOST_OK) return fail("[E::main] %s\n", feed.err);
        if ((rc = phi_reads_collect_end(ctx, nullptr, nullptr))) return fail_on(ctx, "collect", rc);
        if (Stage st("reads scored against every walk"); (rc = phi_reads_collect_score(ctx))) return fail_on(ctx, "reads", rc);
        phi_scout_info si;
        std::vector<uint8_t> always((size_t)n_walks, 0);
        for (int32_t h = 0; h < n_walks; h++)
            always[(size_t)h] = std::find(o.panel_always.begin(), o.panel_always.end(), sample_of(phi_graph_hap_name(g, h))) != o.panel_always.end();
        std::vector<int32_t> round_of((size_t)n_walks, -2);
        keep.assign((size_t)n_walks, 0);
        {
            Stage st("panel from the reads (scores, choice)");
            if ((rc = phi_scout_scores(ctx, o.panel_blocks, nullptr, &si))) return fail_on(ctx, "panel scores", rc);
            if ((rc = phi_scout_choose(ctx, always.data(), o.panel_auto, keep.data(), round_of.data()))) return fail_on(ctx, "panel choice", rc);
        }
        int rounds = 0;
        kept_walks.clear();
        for (int32_t h = 0; h < n_walks; h++) {
            if (keep[(size_t)h]) kept_walks.push_back(h);
            if (round_of[(size_t)h] >= 0 && round_of[(size_t)h] < n_walks) rounds = std::max(rounds, round_of[(size_t)h] + 1);
        }
        stamp("main");
        fprintf(stderr, "Panel (from the reads): kept %d of %d walks in %d rounds over %d blocks:", (int)kept_walks.size(), n_walks, rounds, si.n_blocks);
        for (size_t i = 0; i < kept_walks.size(); i++) fprintf(stderr, "%s%s", i ? "," : " ", phi_graph_hap_name(g, kept_walks[i]));
        fprintf(stderr, "\n");
        {
            Stage st("phi_set_graph_panel (index of the chosen walks)");
            rc = phi_set_graph_panel(ctx, phi_graph_n_vtx(g), phi_graph_seq_concat(g), phi_graph_seq_off(g), phi_graph_adj_off(g), phi_graph_adj(g), n_walks,
                                     auto_walk_off.data(), nullptr, keep.data(), o.chop, PHI_PANEL_RETAIN | PHI_PANEL_KEEP_READS, nullptr);
            if (rc == PHI_ERR_WALK) fprintf(stderr, "Error: %s\n", phi_last_error(ctx));
            if (rc) return fail_on(ctx, "graph", rc);
        }
        walks_retained = true;
        if ((rc = phi_panel_stats(ctx, &panel_info))) return fail_on(ctx, "panel", rc);
        log_panel();
        phi_chop_info ci;
        if (o.chop && !phi_chop_stats(ctx, &ci)) {
            stamp("main");
            fprintf(stderr, "Graph chopped to %d bases: %lld -> %lld vertices, %lld -> %lld walk entries\n", ci.max_len, (long long)ci.n_vtx_in,
                    (long long)ci.n_vtx_out, (long long)ci.n_entries_in, (long long)ci.n_entries_out);
        }
        if (Stage st("reads scored against the panel"); (rc = phi_reads_collect_score(ctx))) return fail_on(ctx, "reads", rc);
        const int status = solve_and_report();
        if (status == 1) return 1;
        if ((rc = phi_reads_collect_release(ctx))) return fail_on(ctx, "collect release", rc);
        return status;
    }
    // ---- stage 1a: walks (ILP_index.cpp:556-611) on every GPU, while the reads are still being read
    int build_index()
    {
        const uint32_t flags = (o.is_qclp ? PHI_FLAG_QCLP : 0) | (o.is_mixed ? PHI_FLAG_MIXED : 0);
        Stage st("phi_set_graph (index build)");
        if (panel_on()) {
            kept_walks.clear();
            for (int32_t h = 0; h < phi_graph_n_walks(g); h++) if (keep[(size_t)h]) kept_walks.push_back(h);
            if (kept_walks.empty()) return fail("[E::main] the panel keeps no walk\n");
        }
        const int rc = run_on_all("graph", [&](int, phi_ctx *cx) -> int {
            // (--panels: a context takes its parameters once, before its first graph)
            int r = walks_retained ? 0 : phi_set_params(cx, o.k, o.w, o.threshold, o.recombination, flags);
            // the reference's model.optimize() has no limit (ILP_index.cpp:1412-1418): none here unless --dp-budget asks for one
            if (!r) r = phi_set_solve_budget(cx, o.dp_budget >= 0 ? o.dp_budget : 0);
            std::vector<int64_t> vcf_walk_off;
            if (!r && vcf && panel_on()) {
                // the graph is built from ALL samples' records; only the kept haplotypes' choice columns become walks, and the
                // panel step, with every walk kept, removes what nobody uses
                const int64_t n_sites = phi_vcf_n_real_sites(vcf);
                const int32_t n_haps = phi_vcf_n_kept_haps(vcf), n_kept = (int32_t)kept_walks.size();
                std::vector<int32_t> choice((size_t)std::max<int64_t>(1, n_sites * n_kept));
                for (int64_t si = 0; si < n_sites; si++)
                    for (int32_t j = 0; j < n_kept; j++) choice[(size_t)(si * n_kept + j)] = phi_vcf_choice(vcf)[si * n_haps + kept_walks[(size_t)j]];
                vcf_walk_off.resize((size_t)n_kept + 1);
                r = phi_vcf_walks(cx, phi_vcf_unit_first(vcf), phi_vcf_n_units(vcf), phi_vcf_site_backbone(vcf), phi_vcf_site_allele0(vcf),
                                  n_sites, choice.data(), n_kept, vcf_walk_off.data());
                const std::vector<uint8_t> all((size_t)n_kept, 1);
                if (!r)
                    r = phi_set_graph_panel(cx, phi_graph_n_vtx(g), phi_graph_seq_concat(g), phi_graph_seq_off(g), phi_graph_adj_off(g), phi_graph_adj(g),
                                            n_kept, vcf_walk_off.data(), nullptr, all.data(), 0, 0, nullptr);
                if (!r && cx == ctx) full_entries = vcf_walk_off[(size_t)n_kept];
            } else if (!r && panel_on()) {
                // --panels: the full entries stay on the device behind the first panel, and every later one starts from them
                const uint32_t pf = panels.empty() ? 0u : PHI_PANEL_RETAIN;
                r = phi_set_graph_panel(cx, phi_graph_n_vtx(g), phi_graph_seq_concat(g), phi_graph_seq_off(g), phi_graph_adj_off(g), phi_graph_adj(g),
                                        phi_graph_n_walks(g), phi_graph_walk_off(g), walks_retained ? nullptr : phi_graph_walk_vtx(g), keep.data(), o.chop, pf,
                                        nullptr);
                if (!r && cx == ctx) full_entries = phi_graph_walk_off(g)[phi_graph_n_walks(g)];
            } else if (!r && vcf) {
                vcf_walk_off.resize((size_t)phi_graph_n_walks(g) + 1);
                r = phi_vcf_walks(cx, phi_vcf_unit_first(vcf), phi_vcf_n_units(vcf), phi_vcf_site_backbone(vcf), phi_vcf_site_allele0(vcf),
                                  phi_vcf_n_real_sites(vcf), phi_vcf_choice(vcf), phi_vcf_n_kept_haps(vcf), vcf_walk_off.data());
                if (!r)
                    r = phi_set_graph(cx, phi_graph_n_vtx(g), phi_graph_seq_concat(g), phi_graph_seq_off(g), phi_graph_adj_off(g),
                                      phi_graph_adj(g), phi_graph_n_walks(g), vcf_walk_off.data(), nullptr, phi_graph_topo_rank(g));
            } else if (!r && o.chop)
                r = phi_set_graph_chopped(cx, phi_graph_n_vtx(g), phi_graph_seq_concat(g), phi_graph_seq_off(g), phi_graph_adj_off(g), phi_graph_adj(g),
                                          phi_graph_n_walks(g), phi_graph_walk_off(g), phi_graph_walk_vtx(g), phi_graph_topo_rank(g), o.chop, nullptr);
            else if (!r)
                r = phi_set_graph(cx, phi_graph_n_vtx(g), phi_graph_seq_concat(g), phi_graph_seq_off(g), phi_graph_adj_off(g),
                                  phi_graph_adj(g), phi_graph_n_walks(g), phi_graph_walk_off(g), phi_graph_walk_vtx(g), phi_graph_topo_rank(g));
            if (r == PHI_ERR_WALK && n_dev == 1) fprintf(stderr, "Error: %s\n", phi_last_error(cx));
            return r;
        });
        if (!rc && panel_on()) {
            if (!panels.empty()) walks_retained = true;
            int prc = phi_panel_stats(ctx, &panel_info);
            if (prc) return fail_on(ctx, "panel", prc);
            log_panel();
        }
        phi_chop_info ci;
        if (!rc && o.chop && !phi_chop_stats(ctx, &ci)) {
            stamp("main");
            fprintf(stderr, "Graph chopped to %d bases: %lld -> %lld vertices, %lld -> %lld walk entries\n", ci.max_len, (long long)ci.n_vtx_in,
                    (long long)ci.n_vtx_out, (long long)ci.n_entries_in, (long long)ci.n_entries_out);
        }
        return rc;
    }
    // The exchange of a multi-GPU run: the library's RCCL all-reduce.  PHI_EXCHANGE=peers takes the peer-mapped OR-gather
    // instead (one kernel per GPU, no RCCL: made for hit vectors of a few MB, every MHC-sized graph) -- opt-in until a run on
    // two or more GPUs has compared the two bit for bit: its cross-GPU loads have only ever run between contexts on ONE GPU.
    int setup_exchange()
    {
        if (n_dev == 1) return 0;
        phi_index_info info;
        int rc;
        if ((rc = phi_index_stats(ctx, &info))) return fail_on(ctx, "index", rc);
        use_peers = kn.exchange_peers;
        if (use_peers && (rc = phi_peers_create(n_dev, &peer_group))) return fail_on(ctx, "peer group", rc);
        Stage st(use_peers ? "peer group (xGMI peer access)" : "RCCL communicator");
        if (!use_peers && (rc = phi_comm_unique_id(comm_id, sizeof comm_id))) return fail("[E::main] RCCL is not available: %s\n", phi_strerror(rc));
        if (run_on_all("communicator", [&](int i, phi_ctx *cx) -> int { return use_peers ? phi_peers_join(cx, peer_group, i) : phi_comm_init(cx, comm_id, i, n_dev); })) return 1;
        fprintf(stderr, "[M::main] %d GPUs; hit vector of %lld flags merged through %s\n", n_dev, (long long)info.n_distinct_minimizers, use_peers ? "peer-mapped memory (one OR-gather kernel per GPU)" : "RCCL all-reduce");
        return 0;
    }

    // The device's text stream on cx ends (under the turn), and what it did not take goes through the host reader.  At the end of
    // the stream (cb == nullptr) that is the file's last record, whose end only the end of the file shows; after text that is not
    // one of the two regular layouts (cb: that chunk, in `slot`) it is the stream from the first byte not taken on.
    int end_on_host(phi_ctx *cx, const Chunk *cb, int slot, bool irr_carry)
    {
        const char *pend = nullptr; int64_t n_pend = 0;
        const int r = phi_reads_text_end(cx, &pend, &n_pend, nullptr);
        std::vector<char> all;
        if (!cb) {
            if (!r && n_dev > 1) { pend = feed.carry.data(); n_pend = (int64_t)feed.carry.size(); }
            if (r || !n_pend) return r;
        } else {
            if (!r && irr_carry) {                            // (the carry, fed as a piece of its own, was what did not fit: this chunk follows it)
                all.assign(pend, pend + n_pend);
                all.insert(all.end(), cb->text, cb->text + cb->n);
                pend = all.data(); n_pend = (int64_t)all.size();
            }
            feed.give_free(slot);
            if (r) return r;
            if (timing) fprintf(stderr, "[phi timing] main: the reads text is not regular FASTA / 4-line FASTQ: host reader from the first byte not taken\n");
        }
        return feed.host_reader(cx, pend, n_pend, cb != nullptr, feed.stream_fed - n_pend);
    }
    // ---- reads (main.cpp:136-137) and stage 1b/2a (:615-655) on one GPU, chunk by chunk.  The chunks are taken in stream order,
    //      one GPU at a time (a chunk needs the unfinished rest of the one before); the sketch of a chunk runs on behind the turn.
    //      Text that is not laid out regularly goes through the host reader from that byte on.
    // ---- a BAM reads file (reads_kind): the same chunks -- the BGZF layer inflated by the host pool, or a single gzip stream by
    //      the device inflater, parked or not -- go to phi_add_reads_bam, which finds and decodes the records on the device
    //      (DESIGN.md 4.14).  One GPU: main refuses a BAM with --devices of several.
    int feed_reads_bam(phi_ctx *cx)
    {
        ReadsFeed &f = feed;
        int r = phi_reads_bam_begin(cx, f.chunk_bytes, Knobs::num("PHI_BAM_TILE", 0));
        const bool open = r == PHI_OK;
        while (!r) {
            const int slot = f.take_full();
            Chunk &cb = *f.at(slot);
            if (cb.n < 0) { r = PHI_ERR_INVALID; fprintf(stderr, "[E::main] %s\n", f.err); break; }
            if (cb.n == 0) break;                             // (the end marker stays in the queue)
            if (++f.n_chunks >= 2) f.pin_buffers(cx);
            f.stream_fed += cb.n;
            if (cb.parked >= 0) {
                r = phi_add_reads_bam_parked(cx, f.park, cb.parked);
                (void)phi_text_park_release(f.park, cb.parked);
            } else r = phi_add_reads_bam(cx, cb.text, cb.n);
            f.give_free(slot);
        }
        phi_bam_info bi;
        if (open) { const int r2 = phi_reads_bam_end(cx, &bi); if (!r) r = r2; }
        if (!r)
            fprintf(stderr, "[M::main] BAM %s: %lld records, %lld reads kept (%lld stored reverse), %lld secondary/supplementary and %lld without sequence dropped; %d reference(s); "
                            "%lld tiles, %lld confirmed, %lld walked again\n", reads_file.c_str(), (long long)bi.n_records, (long long)bi.n_kept, (long long)bi.n_reverse,
                    (long long)bi.n_secondary_supplementary, (long long)bi.n_empty, (int)bi.n_ref, (long long)bi.tiles, (long long)bi.tiles_confirmed, (long long)bi.tiles_rewalked);
        return r;
    }
    int feed_reads(phi_ctx *cx)
    {
        if (reads_kind_now == READS_BAM) return feed_reads_bam(cx);
        ReadsFeed &f = feed;
        int r = phi_reads_text_begin(cx, f.chunk_bytes);
        bool open = r == PHI_OK;
        while (!r) {
            std::unique_lock<std::mutex> turn(f.turn_mu);
            if (f.stream_done || failed) break;
            const int slot = f.take_full();
            Chunk &cb = *f.at(slot);
            int32_t irr_carry = 0, irr = 0;
            if (cb.n < 0) { f.stream_done = true; r = PHI_ERR_INVALID; fprintf(stderr, "[E::main] %s\n", f.err); break; }
            if (cb.n > 0) {
                if (++f.n_chunks >= 2) f.pin_buffers(cx);
                f.stream_fed += cb.n;
                if (n_dev > 1 && !f.carry.empty()) r = phi_add_reads_text(cx, f.carry.data(), (int64_t)f.carry.size(), &irr_carry);
                if (!r && !irr_carry && cb.parked >= 0) {
                    r = phi_add_reads_text_parked(cx, f.park, cb.parked, &irr);
                    if (!r) (void)phi_text_park_release(f.park, cb.parked);
                } else if (!r && !irr_carry) r = phi_add_reads_text(cx, cb.text, cb.n, &irr);
            }
            if (!r && (cb.n == 0 || irr_carry || irr)) {
                // the end of the stream (left in the queue for the other GPUs), or the exact state machine takes the stream
                f.stream_done = true;
                open = false;
                r = end_on_host(cx, cb.n ? &cb : nullptr, slot, irr_carry);
                break;
            }
            const char *p = nullptr; int64_t n = 0;
            if (!r && n_dev > 1 && !(r = phi_reads_text_detach_carry(cx, &p, &n))) f.carry.assign(p, p + n);
            f.give_free(slot);
        }
        if (open) { const int r2 = phi_reads_text_end(cx, nullptr, nullptr, nullptr); if (!r) r = r2; }
        return r;
    }

    // ---- the log (ILP_index.cpp, stages 2b-3), the FASTA (:1577-1598) and the tail of the run
    int report(const phi_result &res)
    {
        const double t_report = realtime();
        const int32_t n_walks = panel_on() ? (int32_t)kept_walks.size() : phi_graph_n_walks(g);      // (the names printed are the kept walks' own)
        int rc;
        fprintf(stderr, "Number of Minimizers\n");
        for (int32_t h = 0; h < n_walks; h++) fprintf(stderr, "%s : %d\n", walk_name(h), (int)res.n_minimizers[h]);
        if (o.debug) {                                        // ILP_index.cpp:591-604
            std::vector<int64_t> hist((size_t)n_walks + 1, 0);
            int64_t n_distinct = 0;
            if ((rc = phi_walk_sharing(ctx, hist.data(), n_walks + 1, &n_distinct))) return fail_on(ctx, "sharing histogram", rc);
            fprintf(stderr, "Shared fraction of unique kmers by haplotypes\n");
            for (int32_t i = 1; i <= n_walks; i++)
                fprintf(stderr, "[Haplotypes: %d, fraction of unique shared kmers: %.5f]\n", i, (float)hist[i] / (float)n_distinct);
        }
        stamp("ILP_function"); fprintf(stderr, "Haplotypes sketched\n");
        stamp("ILP_function"); fprintf(stderr, "Indexed reads with spectrum size: %d\n", (int)res.spectrum_size);
        fprintf(stderr, "Number of Anchors\n");
        for (int32_t h = 0; h < n_walks; h++) fprintf(stderr, "%s : %d\n", walk_name(h), (int)res.n_anchors[h]);
        stamp("ILP_function");
        fprintf(stderr, "Filtered/Retained Minimizers: %.2f/%.2f%%\n", (float)res.filtered / (float)res.spectrum_size * 100, (float)res.retained / (float)res.spectrum_size * 100);
        stamp("ILP_function"); fprintf(stderr, "%s model started\n", o.is_qclp ? "QP" : "ILP");
        stamp("ILP_function"); fprintf(stderr, "%.2f%% Minimizers are in ILP\n", (res.n_in_model * 100.0) / res.spectrum_size);
        stamp("ILP_function"); fprintf(stderr, "Minimizer constraints added to the model\n");
        stamp("ILP_function"); fprintf(stderr, "%s\n", o.is_mixed ? "Using Mixed Integer Programming" : "Using Integer Programming");
        stamp("ILP_function"); fprintf(stderr, "Optimized expanded graph constructed\n");
        stamp("ILP_function"); fprintf(stderr, "Model optimized\n");
        if (o.debug || !res.optimal)
            fprintf(stderr, "[M::%s] objective %lld (upper bound %lld, %s) after %d DP run(s); %lld minimisers covered, %d w-node(s)\n", "solve", (long long)res.objective,
                    (long long)res.upper_bound, res.optimal ? "proven optimal" : "NOT proven optimal", res.n_dp_runs, (long long)res.n_covered, res.n_switches);
        fprintf(stderr, "Recombination count: %d\nRecombined haplotypes: ", res.recombination_count);
        print_recombinations(res);
        g_marks.add("report (log lines)", t_report, realtime());
        {
            Stage st("FASTA write");
            std::unique_ptr<char[]> seq(new char[(size_t)(res.hap_len > 0 ? res.hap_len : 1)]);      // (not zero-filled: every byte is written)
            if ((rc = phi_path_sequence(ctx, seq.get(), res.hap_len))) return fail_on(ctx, "sequence", rc);
            if (o.bgzf) {
                char *text = nullptr;
                int64_t n_text = 0;
                if (phi_format_fasta(hap_name, seq.get(), res.hap_len, &text, &n_text) != PHI_HOST_OK) return fail("[E::main] cannot format %s\n", hap_file.c_str());
                seq.reset();
                int wrc = write_bgzf(hap_file, text, n_text, o.bgzf_index ? PHI_BGZF_INDEX_GZI : 0);
                phi_host_free_text(text);
                if (!wrc && o.bgzf_index) wrc = write_fai(hap_file + ".fai", hap_name, res.hap_len);
                if (wrc) return 1;
            } else if (phi_write_fasta(hap_file.c_str(), hap_name, seq.get(), res.hap_len) != PHI_HOST_OK) return fail("[E::main] cannot write %s\n", hap_file.c_str());
        }
        stamp("ILP_function"); fprintf(stderr, "Haplotype of size: %d written to: %s\n", (int)res.hap_len, hap_file.c_str());
        if (!o.calls_files.empty() && write_calls(res)) return 1;
        fprintf(stderr, "[M::%s] PHI Version: %s\n[M::%s] CMD:", "main", PHI_VERSION, "main");
        for (int i = 0; i < o.argc; ++i) fprintf(stderr, " %s", o.argv[i]);
        fprintf(stderr, "\n[M::%s] Real time: %.3f sec; CPU: %.3f sec; Peak RSS: %.3f GB\n", "main", realtime() - t0_real, cputime(), peakrss() / 1024.0 / 1024.0 / 1024.0);
        if (!timing) return 0;
        if (feed.parked_bytes) fprintf(stderr, "[phi timing] main: %lld bytes of the reads text waited in device memory for the index\n", (long long)feed.parked_bytes);
        const phi_inflate_info &inf = feed.inflated;
        if (inf.out_bytes)
            fprintf(stderr, "[phi timing] main: %lld bytes inflated on the device from %lld gzip bytes (%lld chunks: %lld confirmed at their start, %lld decoded again)\n",
                    (long long)inf.out_bytes, (long long)inf.in_bytes, (long long)inf.chunks, (long long)inf.confirmed, (long long)inf.redecoded);
        fprintf(stderr, "[phi timing] main: %d text chunk(s) of up to %lld bytes%s on %d GPU(s); %lld bases through the host reader; FASTA closed at epoch %.6f%s\n",
                feed.n_chunks.load(), (long long)feed.chunk_bytes, feed.n_chunks >= 2 && feed.pinned ? ", pinned" : "", n_dev, (long long)feed.host_bases, realtime(),
                o.detached ? "; teardown detached" : "");
        g_marks.print();
        print_resident();
        return 0;
    }
    // ---- --calls: the reference walk among the context's walks (after a panel: the kept ones, through phi_panel_walks' ids).
    //      1 with a message when the graph holds no such walk or the panel has dropped it: never another walk silently
    int calls_ref_walk(int32_t *out)
    {
        const std::string want = !o.calls_ref.empty() ? o.calls_ref : "REF.0";      // (main refuses -g without --calls-ref)
        int32_t in_g = -1;
        for (int32_t h = 0; h < phi_graph_n_walks(g) && in_g < 0; h++)
            if (want == phi_graph_hap_name(g, h)) in_g = h;
        if (in_g < 0) return fail("[E::main] --calls-ref %s: the graph holds no walk of that name (walks are named SAMPLE.HAP, as the log prints them)\n", want.c_str());
        if (!panel_on()) { *out = in_g; return 0; }
        for (size_t k = 0; k < kept_walks.size(); k++)
            if (kept_walks[k] == in_g) { *out = (int32_t)k; return 0; }
        return fail("[E::main] --calls-ref %s: the panel does not keep this walk, and calls are made against no other; keep it with --panel-always %s (or --keep-samples)\n",
                    want.c_str(), sample_of(want.c_str()).c_str());
    }
    static bool write_all(const std::string &file, const void *p, int64_t n)
    {
        FILE *fp = fopen(file.c_str(), "wb");
        bool ok = fp && fwrite(p, 1, (size_t)n, fp) == (size_t)n;
        if (fp && fclose(fp) != 0) ok = false;
        return ok;
    }
    // --bgzf: text[0, n) compressed into BGZF blocks on the command's device (phi_deflate_bgzf), written under the name as given.
    // --bgzf-index (index_kind, 0 without): its index built with it (phi_deflate_bgzf_indexed) and written to FILE.gzi / FILE.tbi
    int write_bgzf(const std::string &file, const char *text, int64_t n, int32_t index_kind)
    {
        void *z = nullptr, *x = nullptr;
        int64_t zn = 0, xn = 0;
        phi_deflate_info di;
        phi_bgzf_index_info xi;
        if (index_kind) {
            const int rc = phi_deflate_bgzf_indexed(devices[0], text, n, 0, index_kind, &z, &zn, &x, &xn, &di, &xi);
            if (rc) return fail("[E::main] --bgzf-index %s: %s: %s\n", file.c_str(), phi_strerror(rc), xi.detail);
        } else {
            const int rc = phi_deflate_bgzf_alloc(devices[0], text, n, 0, &z, &zn, &di);
            if (rc) return fail("[E::main] --bgzf %s: %s: %s\n", file.c_str(), phi_strerror(rc), di.detail);
        }
        const std::string index_file = file + (index_kind == PHI_BGZF_INDEX_GZI ? ".gzi" : ".tbi");
        const bool ok = write_all(file, z, zn), ok_index = !index_kind || write_all(index_file, x, xn);
        phi_deflate_free(z);
        phi_deflate_free(x);
        if (!ok || !ok_index) return fail("[E::main] cannot write %s\n", ok ? index_file.c_str() : file.c_str());
        stamp("main");
        fprintf(stderr, "BGZF: %lld bytes written to %s, %lld bytes of text in %lld blocks (%lld stored); %.3f ms on device %d\n", (long long)zn, file.c_str(),
                (long long)di.in_bytes, (long long)di.blocks, (long long)di.stored_blocks, di.device_ms, devices[0]);
        if (index_kind) {
            stamp("main");
            fprintf(stderr, "BGZF index: %lld bytes written to %s, %lld records on %lld contigs, %lld chunks, %lld windows; %.3f ms on device %d\n", (long long)xn,
                    index_file.c_str(), (long long)xi.records, (long long)xi.contigs, (long long)xi.chunks, (long long)xi.windows, xi.device_ms, devices[0]);
        }
        return 0;
    }
    // --bgzf-index: the .fai of a FASTA that phi_format_fasta made; with the .gzi a reader finds any base without inflating the rest
    int write_fai(const std::string &file, const char *name, int64_t len)
    {
        char *line = nullptr;
        int64_t n_line = 0;
        if (phi_format_fasta_fai(name, len, &line, &n_line) != PHI_HOST_OK) return fail("[E::main] cannot format %s\n", file.c_str());
        const bool ok = write_all(file, line, n_line);
        phi_host_free_text(line);
        if (!ok) return fail("[E::main] cannot write %s\n", file.c_str());
        stamp("main");
        fprintf(stderr, "BGZF index: %lld bytes written to %s, 1 records on 1 contigs, 0 chunks, 0 windows; 0.000 ms on device %d\n", (long long)n_line, file.c_str(), devices[0]);
        return 0;
    }
    // the path of the solve just reported as calls against the reference walk, written beside the FASTA
    int write_calls(const phi_result &res)
    {
        std::string file = o.calls_files[(size_t)job_now];
        for (size_t at; !cov_now.empty() && (at = file.find("{cov}")) != std::string::npos;) file.replace(at, 5, cov_now);
        for (size_t at; !panel_now.empty() && (at = file.find("{panel}")) != std::string::npos;) file.replace(at, 7, panel_now);
        int32_t r = 0;
        if (calls_ref_walk(&r)) return 1;
        Stage st("calls (device) + VCF write");
        phi_calls cl;
        phi_calls_info ci;
        int rc;
        if ((rc = phi_calls_path(ctx, r, &cl)) || (rc = phi_calls_stats(ctx, &ci))) return fail_on(ctx, "calls", rc);
        phi_call_support sup{};                               // --calls-support: the read support of every call, counted behind the calls
        if (o.calls_support) {
            Stage ss("calls support (device)");
            if ((rc = phi_calls_support(ctx, &sup))) return fail_on(ctx, "calls support", rc);
        }
        const char *ref_name = walk_name(r);
        const bool vcf_ref = o.from_vcf && !strcmp(ref_name, "REF.0");
        const std::string contig = !o.calls_contig.empty() ? o.calls_contig : vcf_ref ? phi_vcf_contig(vcf) : ref_name;
        const int64_t contig_len = vcf_ref ? (o.region.empty() ? phi_vcf_ref_len(vcf) : region_contig_len) : ci.ref_bases;
        std::vector<int64_t> shifted;                         // --region: the records in the contig's coordinates, POS plus the region's origin
        if (vcf_ref && !o.region.empty() && phi_vcf_origin(vcf) != 0) {
            shifted.assign(cl.pos, cl.pos + cl.n_calls);
            for (int64_t &p : shifted) p += phi_vcf_origin(vcf);
            cl.pos = shifted.data();
        }
        std::vector<const char *> ph((size_t)cl.n_calls);
        for (int64_t k = 0; k < cl.n_calls; k++) ph[(size_t)k] = walk_name(res.path_hap[cl.anchor[k] + 1]);
        int64_t n_written = 0, n_dropped = 0;
        char werr[512] = "";
        if (o.bgzf) {
            char *text = nullptr;
            int64_t n_text = 0;
            const int frc = o.calls_support
                                ? phi_format_calls_vcf_support(contig.c_str(), contig_len, hap_name, cl.n_calls, cl.pos, cl.ref_off, cl.ref_bytes, cl.alt_off, cl.alt_bytes,
                                                               ph.data(), sup.alt_hit, sup.alt_n, sup.ref_hit, sup.ref_n, &text, &n_text, &n_written, &n_dropped, werr, sizeof werr)
                                : phi_format_calls_vcf(contig.c_str(), contig_len, hap_name, cl.n_calls, cl.pos, cl.ref_off, cl.ref_bytes, cl.alt_off, cl.alt_bytes, ph.data(),
                                                       &text, &n_text, &n_written, &n_dropped, werr, sizeof werr);
            if (frc != PHI_HOST_OK)
                return fail("[E::main] %s\n", werr[0] ? werr : "cannot format the calls");
            const int wrc = write_bgzf(file, text, n_text, o.bgzf_index ? PHI_BGZF_INDEX_TBI_VCF : 0);
            phi_host_free_text(text);
            if (wrc) return 1;
        } else if ((o.calls_support
                        ? phi_write_calls_vcf_support(file.c_str(), contig.c_str(), contig_len, hap_name, cl.n_calls, cl.pos, cl.ref_off, cl.ref_bytes, cl.alt_off,
                                                      cl.alt_bytes, ph.data(), sup.alt_hit, sup.alt_n, sup.ref_hit, sup.ref_n, &n_written, &n_dropped, werr, sizeof werr)
                        : phi_write_calls_vcf(file.c_str(), contig.c_str(), contig_len, hap_name, cl.n_calls, cl.pos, cl.ref_off, cl.ref_bytes, cl.alt_off, cl.alt_bytes,
                                              ph.data(), &n_written, &n_dropped, werr, sizeof werr)) != PHI_HOST_OK)
            return fail("[E::main] %s\n", werr[0] ? werr : "cannot write the calls");
        stamp("main");
        if (o.calls_support)
            fprintf(stderr, "Call support: %lld calls, %lld of %lld ALT and %lld of %lld REF witness minimisers seen\n", (long long)sup.n_calls,
                    (long long)sup.alt_hit_total, (long long)sup.alt_n_total, (long long)sup.ref_hit_total, (long long)sup.ref_n_total);
        fprintf(stderr, "Calls: %lld written to %s, %lld dropped as REF = ALT; called span [%lld,%lld) of %s (%lld bases), [%lld,%lld) of the haplotype\n",
                (long long)n_written, file.c_str(), (long long)n_dropped, (long long)cl.ref_span[0], (long long)cl.ref_span[1], ref_name, (long long)ci.ref_bases,
                (long long)cl.query_span[0], (long long)cl.query_span[1]);
        return 0;
    }
    // ---- recombination report (:1508-1550): segments in output coordinates
    void print_recombinations(const phi_result &res)
    {
        const int64_t *so = phi_graph_seq_off(g);
        int64_t str_id = 0, prev_str_id = 0;
        int32_t prev_hap = res.n_path ? res.path_hap[0] : 0;
        // --chop: the path's vertices are pieces; their segments and offsets, so that the lengths come from g's segments
        std::vector<int32_t> seg, at;
        if (o.chop) {
            seg.resize((size_t)res.n_path); at.resize((size_t)res.n_path);
            const int rc = phi_chop_origin(ctx, res.path_vtx, res.n_path, seg.data(), at.data());
            if (rc) { fprintf(stderr, "\n[E::main] recombination report: %s: %s\n", phi_strerror(rc), phi_last_error(ctx)); return; }
        }
        // a panel: the (unchopped) vertices are the panel graph's; g's own through phi_panel_origin
        std::vector<int32_t> orig;
        if (panel_on()) {
            orig.resize((size_t)res.n_path);
            const int rc = phi_panel_origin(ctx, o.chop ? seg.data() : res.path_vtx, res.n_path, orig.data());
            if (rc) { fprintf(stderr, "\n[E::main] recombination report: %s: %s\n", phi_strerror(rc), phi_last_error(ctx)); return; }
        }
        for (int64_t i = 0; i < res.n_path; i++) {
            const int32_t v = panel_on() ? orig[(size_t)i] : o.chop ? seg[(size_t)i] : res.path_vtx[i];
            const int64_t len = o.chop ? std::max<int64_t>(0, std::min<int64_t>(o.chop, so[v + 1] - so[v] - at[(size_t)i])) : so[v + 1] - so[v];
            str_id += len;                                    // (the reference adds the vertex length before testing the label: :1515-1523)
            if (i > 0 && res.path_hap[i] != prev_hap) {
                fprintf(stderr, ">(%s,[%lld,%lld])", walk_name(prev_hap), (long long)prev_str_id, (long long)(str_id - 1));
                prev_hap = res.path_hap[i]; prev_str_id = str_id;
            }
        }
        if (res.n_path) fprintf(stderr, ">(%s,[%lld,%lld])", walk_name(prev_hap), (long long)prev_str_id, (long long)(str_id - 1));
        fprintf(stderr, "\n");
    }
    // what the peak is made of: the mapped GFA file's own pages count as resident (RssFile / RssShmem), anonymous memory is the rest
    static void print_resident()
    {
        FILE *fp = fopen("/proc/self/status", "r");
        if (!fp) return;
        char line[256];
        long hwm = -1, anon = -1, file = -1, shm = -1;
        while (fgets(line, sizeof line, fp)) {
            if (!strncmp(line, "VmHWM:", 6)) hwm = atol(line + 6);
            else if (!strncmp(line, "RssAnon:", 8)) anon = atol(line + 8);
            else if (!strncmp(line, "RssFile:", 8)) file = atol(line + 8);
            else if (!strncmp(line, "RssShmem:", 9)) shm = atol(line + 9);
        }
        fclose(fp);
        fprintf(stderr, "[phi timing] main: resident now: anonymous %.3f GB, mapped files %.3f GB (the GFA among them); peak %.3f GB\n", anon / 1048576.0, (file + shm) / 1048576.0, hwm / 1048576.0);
    }
    // ---- one read set against the graph and its index: 0, 3 (the path is not proven optimal) or 1 (an error)
    int run_job(int job, bool first_of_run = false)
    {
        if (job > 0 || !first_of_run) {
            // the next read set: clocks, names, the chunk queue and the reader thread start over; the contexts forget the reads
            fflush(nullptr);
            const double now = realtime();
            cpu0 += cputime(); t0_real = now;
            g_marks.clear();
            reads_file = o.reads_files[(size_t)job]; hap_file = o.hap_files[(size_t)job];
            reads_kind_now = o.reads_kinds[(size_t)job];
            if (name_job()) return 1;
            feed.start(reads_file);
            if (run_on_all("reset", [&](int, phi_ctx *cx) -> int { return phi_reset_reads(cx); })) return 1;
            loaded();
        }
        if (!hap_pattern.empty()) hap_file = hap_pattern;
        job_now = job;
        if (auto_on) {                                        // (--panel-auto: the scout again for a further read set, from the retained entries)
            if ((job > 0 || !first_of_run) && scout_index()) return 1;
            return run_auto_job();
        }
        const bool ladder = !o.cov.empty();                  // (one GPU: main refuses --coverage with --devices of several)
        int rc;
        if (ladder && (rc = phi_reads_collect_begin(ctx, 0))) return fail_on(ctx, "collect", rc);
        if (Stage st("reads: text -> device, records, sketch"); run_on_all("reads", [&](int, phi_ctx *cx) -> int { return feed_reads(cx); })) return 1;
        if (feed.reader.get() != PHI_HOST_OK) return fail("[E::main] %s\n", feed.err);
        if (ladder) return run_ladder();
        if (n_dev > 1) {
            Stage st(use_peers ? "exchange (peer-mapped)" : "exchange (RCCL)");
            if (run_on_all("exchange", [&](int, phi_ctx *cx) -> int { return use_peers ? phi_peers_exchange(cx) : phi_comm_exchange(cx); })) return 1;
        }
        return solve_and_report();
    }
    // ---- the read set as collected: plan, then per level advance, solve, FASTA (what a plain run logs, behind one line per level)
    int run_ladder()
    {
        int rc, status = 0;
        int64_t n_reads = 0, n_bases = 0;
        if ((rc = phi_reads_collect_end(ctx, &n_reads, &n_bases))) return fail_on(ctx, "collect", rc);
        std::vector<double> fr;
        for (double cv : o.cov) fr.push_back(n_bases > 0 ? std::min(1.0, cv * o.genome_size / (double)n_bases) : 1.0);
        phi_ladder_info li;
        if (Stage st("ladder plan (count, scan, scatter, copy)"); (rc = phi_ladder_plan(ctx, o.seed, fr.data(), (int32_t)fr.size(), &li))) return fail_on(ctx, "ladder plan", rc);
        const std::string pattern = hap_file;
        int64_t lr = 0, lb = 0;
        for (size_t j = 0; j < fr.size(); j++) {
            if (Stage st("ladder advance"); (rc = phi_ladder_advance(ctx, (int32_t)j))) return fail_on(ctx, "ladder advance", rc);
            lr += li.band_reads[j]; lb += li.band_bases[j];
            hap_file = pattern;
            for (size_t at; (at = hap_file.find("{cov}")) != std::string::npos;) hap_file.replace(at, 5, o.cov_names[j]);
            cov_now = o.cov_names[j];
            fprintf(stderr, "Coverage %sx: fraction %.6f, %lld reads, %lld bases\n", o.cov_names[j].c_str(), fr[j], (long long)lr, (long long)lb);
            const int r = solve_and_report();
            if (r == 1) return 1;
            if (r) status = r;
        }
        hap_file = pattern;
        cov_now.clear();
        if ((rc = phi_reads_collect_release(ctx))) return fail_on(ctx, "collect release", rc);
        return status;
    }
    int solve_and_report()
    {
        int64_t total_reads = 0;
        int rc;
        for (phi_ctx *cx : ctxs) {
            int64_t nr = 0;
            if ((rc = phi_reads_stats(cx, &nr, nullptr, nullptr, nullptr))) return fail_on(cx, "reads", rc);
            total_reads += nr;
        }
        stamp("ILP_function"); fprintf(stderr, "Graph has %d vertices, %d walks and read has %d reads\n", panel_on() ? (int)panel_info.n_vtx_out : phi_graph_n_vtx(g),
                                      panel_on() ? (int)kept_walks.size() : phi_graph_n_walks(g), (int)total_reads);
        if (int32_t r = 0; !o.calls_files.empty() && calls_ref_walk(&r)) return 1;      // (a --calls-ref the panel dropped: before the solve)
        phi_result res;
        if (Stage st("phi_solve (filter, exact solve, decode)"); (rc = phi_solve(ctx, &res))) return fail_on(ctx, "solve", rc);
        if (report(res)) return 1;
        if (res.optimal) return 0;
        // the reference returns only what model.optimize() proved (ILP_index.cpp:1418); here that can only fall short when
        // --dp-budget set a limit: the path written is feasible and within the printed bound, the exit status says so
        fprintf(stderr, "[W::main] the path written is NOT proven optimal: the exact search used its budget of %d DP runs (objective %lld, proven upper bound %lld); "
                        "raise it with --dp-budget N (0 = no limit, the default)\n", res.n_dp_runs, (long long)res.objective, (long long)res.upper_bound);
        return 3;
    }
    // PHI_FULL_TEARDOWN (leak checks): everything given back in order
    void teardown() { feed.stop_reader(); feed.teardown(ctx); phi_graph_free(g); if (vcf) phi_vcf_free(vcf); for (phi_ctx *cx : ctxs) phi_ctx_destroy(cx); }
};

// Every stage keeps its overlap: the device contexts are made while the GFA is parsed, the reads file is read while the graph
// loads, its text is parked in device memory only between the GFA parsed and the index built, and the device inflater waits
// for the GFA parsed.
static int run(const Options &o)
{
    Driver d(o);
    const Knobs &kn = d.kn;
    std::vector<int> &devices = d.devices;
    if (devices.empty()) devices.push_back(o.device);
    for (size_t i = 0; i < devices.size(); i++)
        for (size_t j = 0; j < i; j++)
            if (devices[i] == devices[j] && !kn.allow_same_device) { fprintf(stderr, "[E::main] --devices names GPU %d twice\n", devices[i]); return 1; }
    // a read set is sharded only over as many GPUs as it can keep busy: every further GPU costs an exchange (~tens of
    // microseconds) and an index build, and one GPU scores 50 Mbases in a fifth of a millisecond
    if (const FileProbe p = devices.size() > 1 ? probe_file(d.reads_file) : FileProbe(); p.regular) {
        const long long bytes = (long long)p.size;
        const size_t want = (size_t)std::max<long long>(1, (bytes + o.shard_min_bases - 1) / std::max<long long>(1, o.shard_min_bases));
        if (want < devices.size()) {
            fprintf(stderr, "[M::main] reads file of %lld bytes: using %zu of the %zu GPUs given (--shard-min-bases %lld per GPU)\n", bytes, want, devices.size(), o.shard_min_bases);
            devices.resize(want);
        }
    }
    const int n_dev = d.n_dev = (int)devices.size();

    // The device context (HIP initialisation) and the reads file are prepared by two host threads while this one parses the
    // graph: the three are independent.  One host thread per GPU: each context initialises its own device.
    d.ctxs.assign((size_t)n_dev, nullptr);
    d.f_ctx = std::async(std::launch::async, [&d, n_dev]() {
        Stage st("device context(s) [thread]");
        std::vector<std::future<int>> fs;
        for (int i = 0; i < n_dev; i++)
            fs.push_back(std::async(std::launch::async, [&d, i]() { return phi_ctx_create(d.devices[(size_t)i], &d.ctxs[(size_t)i]); }));
        int r = 0;
        for (auto &f : fs) { const int ri = f.get(); if (ri && !r) r = ri; }
        return r;
    }).share();
    const FileProbe rp = probe_file(d.reads_file);
    if (!d.feed.alloc(&kn, devices[0], chunk_size(kn, o.reads_files), 2 + n_dev, n_dev == 1 && kn.text_park && rp.regular && rp.size >= kn.text_park_min,
                      n_dev == 1 && kn.inflate))
        { fprintf(stderr, "[E::%s] out of memory\n", __func__); return 1; }
    d.feed.start(d.reads_file);

    if (d.load_graph()) return 1;
    d.loaded();
    if (d.name_job()) return 1;
    int rc;
    if (Stage st("wait for the device context"); (rc = d.f_ctx.get())) return d.fail("[E::main] no usable MI355X (HIP) device %d: %s\n", devices[0], phi_strerror(rc));
    d.ctx = d.ctxs[0];
    if (d.plan_panels()) return 1;
    // --panels: the graph file is parsed once and its walks go to the device once; every panel is set, scored and solved in
    // turn (the reads stage runs again per panel: phi_set_graph drops what a context has seen of the reads, on purpose)
    const size_t n_panels = std::max<size_t>(1, d.panels.size());
    int status = 0;
    for (size_t pj = 0; pj < n_panels; pj++) {
        if (!d.panels.empty()) d.mask_of(d.panels[pj], false);
        if (d.auto_on ? d.scout_index() : d.build_index()) return 1;
        d.feed.mark(d.feed.index_built);                     // (the reader thread stops parking chunks: they are taken as they come now)
        if (pj == 0 && d.setup_exchange()) return 1;
        // ---- one job per read set (-r a -o a.fa -r b -o b.fa ...): the graph, its index and the communicator are made once
        for (int job = 0; job < (int)o.reads_files.size(); job++) {
            if (!d.panels.empty()) {
                d.hap_pattern = o.hap_files[(size_t)job];
                for (size_t at; (at = d.hap_pattern.find("{panel}")) != std::string::npos;) d.hap_pattern.replace(at, 7, o.panel_names[pj]);
                d.panel_now = o.panel_names[pj];
            }
            const int r = d.run_job(job, pj == 0 && job == 0);
            if (r == 1) return 1;
            if (r) status = r;
        }
    }
    if (d.walks_retained) for (phi_ctx *cx : d.ctxs) (void)phi_panel_release(cx);
    if (kn.full_teardown) d.teardown();
    return status;
}

int main(int argc, char *argv[])
{
    Options o;
    int help = 0;
    static struct option long_options[] = {{"version", no_argument, 0, 300}, {"device", required_argument, 0, 301}, {"dp-budget", required_argument, 0, 302},
                                           {"devices", required_argument, 0, 303}, {"shard-min-bases", required_argument, 0, 304}, {"chop", required_argument, 0, 305}, {"vcf", required_argument, 0, 306}, {"ref", required_argument, 0, 307},
                                           {"coverage", required_argument, 0, 308}, {"genome-size", required_argument, 0, 309}, {"seed", required_argument, 0, 310},
                                           {"keep-samples", required_argument, 0, 311}, {"drop-samples", required_argument, 0, 312}, {"panels", required_argument, 0, 313},
                                           {"panel-seed", required_argument, 0, 314}, {"panel-always", required_argument, 0, 315},
                                           {"panel-auto", required_argument, 0, 316}, {"panel-blocks", required_argument, 0, 317},
                                           {"calls", required_argument, 0, 318}, {"calls-ref", required_argument, 0, 319}, {"calls-contig", required_argument, 0, 320}, {"bgzf", no_argument, 0, 321}, {"calls-support", no_argument, 0, 322}, {"bgzf-index", no_argument, 0, 323}, {"region", required_argument, 0, 324}, {0, 0, 0, 0}};
    int c;
    std::string gfa_arg, vcf_arg;
    // main.cpp:38 declares -h with an argument; a bare -h falls into the usage branch either way
    while ((c = getopt_long(argc, argv, "x:d:c:l:s:m:R:q:T:N:h:k:w:t:g:r:o:DS", long_options, nullptr)) >= 0) {
        if (c == 'w') o.w = atoi(optarg);
        else if (c == 'k') o.k = atoi(optarg);
        else if (c == 't') o.n_threads = atoi(optarg);
        else if (c == 'm') o.is_mixed = atoi(optarg);
        else if (c == 'g') { gfa_arg = optarg; }
        else if (c == 306) { vcf_arg = optarg; }
        else if (c == 307) o.vcf_ref = optarg;
        else if (c == 324) o.region = optarg;
        else if (c == 'R') o.recombination = atoi(optarg);
        else if (c == 'q') o.is_qclp = atoi(optarg);
        else if (c == 'N') o.is_naive = atoi(optarg);
        else if (c == 'T') o.threshold = (float)atof(optarg);
        else if (c == 'r') { o.reads_file = optarg; o.reads_files.push_back(optarg); }
        else if (c == 'o') { o.hap_file = optarg; o.hap_files.push_back(optarg); }
        else if (c == 'c') o.max_occ = atoi(optarg);
        else if (c == 'd') o.debug = atoi(optarg);
        else if (c == 'h' || c == '?') help = 1;
        else if (c == 300) { fprintf(stderr, "PHI version: %s\n", PHI_VERSION); return 0; }
        else if (c == 301) o.device = atoi(optarg);
        else if (c == 302) o.dp_budget = atoll(optarg);
        else if (c == 305) { o.chop = atoi(optarg); if (o.chop < 1) { fprintf(stderr, "[E::main] --chop takes a segment length of at least 1\n"); return 1; } }
        else if (c == 308) {                                   // --coverage 0.1,0.5,1,...: ascending
            o.cov.clear(); o.cov_names.clear();
            for (const char *p = optarg; *p;) {
                char *end = nullptr;
                const double v = strtod(p, &end);
                if (end == p || !(v >= 0.0) || (*end && *end != ',')) { fprintf(stderr, "[E::main] --coverage takes a comma-separated list of coverages, e.g. 0.1,0.5,1,2,5,10,15\n"); return 1; }
                if (!o.cov.empty() && v < o.cov.back()) { fprintf(stderr, "[E::main] --coverage: the coverages must ascend (%s follows %s)\n", std::string(p, (const char *)end).c_str(), o.cov_names.back().c_str()); return 1; }
                o.cov.push_back(v); o.cov_names.emplace_back(p, (const char *)end);
                p = *end == ',' ? end + 1 : end;
            }
            if (o.cov.empty() || o.cov.size() > 16) { fprintf(stderr, "[E::main] --coverage takes 1 to 16 coverages\n"); return 1; }
        }
        else if (c == 309) o.genome_size = atof(optarg);
        else if (c == 310) o.seed = strtoull(optarg, nullptr, 10);
        else if (c == 311 || c == 312 || c == 315) {
            std::vector<std::string> &names = c == 311 ? o.keep_samples : c == 312 ? o.drop_samples : o.panel_always;
            const char *opt = c == 311 ? "--keep-samples" : c == 312 ? "--drop-samples" : "--panel-always";
            if (!read_names(optarg, names)) { fprintf(stderr, "[E::main] %s: cannot read %s\n", opt, optarg + 1); return 1; }
            if (names.empty()) { fprintf(stderr, "[E::main] %s takes sample names: A,B,.. or @FILE with one name per line\n", opt); return 1; }
            if (c == 311) o.have_keep = true;
            if (c == 312) o.have_drop = true;
        }
        else if (c == 313) {                                   // --panels 3,6,12,24: ascending counts of samples besides the always-kept ones
            o.panel_sizes.clear(); o.panel_names.clear();
            for (const char *p = optarg; *p;) {
                char *end = nullptr;
                const long v = strtol(p, &end, 10);
                if (end == p || v < 0 || v > 1000000 || (*end && *end != ',')) { fprintf(stderr, "[E::main] --panels takes a comma-separated list of sample counts, e.g. 3,6,12,24\n"); return 1; }
                if (!o.panel_sizes.empty() && v < o.panel_sizes.back()) { fprintf(stderr, "[E::main] --panels: the sizes must ascend (%ld follows %d)\n", v, o.panel_sizes.back()); return 1; }
                o.panel_sizes.push_back((int)v); o.panel_names.emplace_back(p, (const char *)end);
                p = *end == ',' ? end + 1 : end;
            }
            if (o.panel_sizes.empty() || o.panel_sizes.size() > 16) { fprintf(stderr, "[E::main] --panels takes 1 to 16 sizes\n"); return 1; }
        }
        else if (c == 314) o.panel_seed = strtoull(optarg, nullptr, 10);
        else if (c == 316) { o.panel_auto = atoi(optarg); if (o.panel_auto < 1 || o.panel_auto > 1022) { fprintf(stderr, "[E::main] --panel-auto takes the number of walks to keep, 1 to 1022\n"); return 1; } }
        else if (c == 317) { o.panel_blocks = atoi(optarg); if (o.panel_blocks < 1 || o.panel_blocks > 65536) { fprintf(stderr, "[E::main] --panel-blocks takes a number of blocks, 1 to 65536\n"); return 1; } }
        else if (c == 318) o.calls_files.push_back(optarg);
        else if (c == 319) o.calls_ref = optarg;
        else if (c == 320) o.calls_contig = optarg;
        else if (c == 321) o.bgzf = true;
        else if (c == 323) o.bgzf_index = true;
        else if (c == 322) o.calls_support = true;
        else if (c == 304) o.shard_min_bases = std::max<long long>(1, atoll(optarg));
        else if (c == 303) {                                   // --devices 0,1,2,...: shard the reads over these GPUs
            o.devices.clear();
            for (const char *p = optarg; *p;) {
                char *end = nullptr;
                const long d = strtol(p, &end, 10);
                if (end == p || d < 0) { fprintf(stderr, "[E::main] --devices takes a comma-separated list of GPU ordinals\n"); return 1; }
                o.devices.push_back((int)d);
                p = *end == ',' ? end + 1 : end;
                if (*end && *end != ',') { fprintf(stderr, "[E::main] --devices takes a comma-separated list of GPU ordinals\n"); return 1; }
            }
        }
    }
    if (!vcf_arg.empty() && !gfa_arg.empty()) { fprintf(stderr, "[E::main] --vcf and -g exclude each other: the graph comes from a GFA or from a VCF + FASTA\n"); return 1; }
    if (vcf_arg.empty() != o.vcf_ref.empty()) { fprintf(stderr, "[E::main] --vcf FILE and --ref FILE go together (a phased VCF and its reference FASTA)\n"); return 1; }
    if (!o.region.empty() && vcf_arg.empty()) { fprintf(stderr, "[E::main] --region R goes with --vcf FILE --ref FILE: a region of an indexed VCF and FASTA (a GFA has no index to read it through)\n"); return 1; }
    o.gfa_file = vcf_arg.empty() ? gfa_arg : vcf_arg;
    if (!vcf_arg.empty()) { o.from_vcf = true; o.vcf_max_len = o.chop ? o.chop : 30; o.chop = 0; }      // (--chop N: the segments are built at that length)
    if (argc < 2 || o.gfa_file.empty() || o.reads_file.empty() || o.hap_file.empty() || help) {
        usage(stderr, o.k, o.w, o.recombination, o.is_qclp, o.is_mixed, o.threshold, o.n_threads, o.gfa_file.c_str(), o.reads_file.c_str(), o.hap_file.c_str(), o.debug);
        return 1;
    }
    if (o.reads_files.size() != o.hap_files.size()) { fprintf(stderr, "[E::main] %zu -r but %zu -o: several read sets against one graph are given as -r a.fq -o a.fa -r b.fq -o b.fa ...\n", o.reads_files.size(), o.hap_files.size()); return 1; }
    for (const std::string &rf : o.reads_files) {
        const ReadsKind kind = reads_kind(rf);
        o.reads_kinds.push_back((int)kind);
        if (kind == READS_CRAM) { fprintf(stderr, "[E::main] %s is a CRAM file: reads are taken from FASTA, FASTQ and BAM; convert it first (samtools view -b, or samtools fastq)\n", rf.c_str()); return 1; }
        if (kind == READS_SAM) { fprintf(stderr, "[E::main] %s is SAM text: reads are taken from FASTA, FASTQ and BAM; convert it first (samtools view -b, or samtools fastq)\n", rf.c_str()); return 1; }
        if (kind == READS_BAM && o.devices.size() > 1) { fprintf(stderr, "[E::main] %s is a BAM file: BAM reads run on one GPU, not together with --devices of several (a BAM is not sharded over contexts)\n", rf.c_str()); return 1; }
    }
    if (!o.cov.empty()) {
        if (!(o.genome_size > 0.0)) { fprintf(stderr, "[E::main] --coverage needs --genome-size N (the bases of the region the coverages refer to)\n"); return 1; }
        if (o.devices.size() > 1) { fprintf(stderr, "[E::main] --coverage runs on one GPU: not together with --devices of several (sharded ladders are not supported)\n"); return 1; }
        if (o.cov.size() > 1)
            for (const std::string &h : o.hap_files)
                if (h.find("{cov}") == std::string::npos) { fprintf(stderr, "[E::main] --coverage with several coverages: -o must contain {cov} (got %s), e.g. -o 'out.{cov}x.fa'\n", h.c_str()); return 1; }
    } else if (o.genome_size != 0.0) { fprintf(stderr, "[E::main] --genome-size goes with --coverage\n"); return 1; }
    if ((int)o.have_keep + (int)o.have_drop + (int)!o.panel_sizes.empty() > 1) { fprintf(stderr, "[E::main] --keep-samples, --drop-samples and --panels exclude each other\n"); return 1; }
    if (o.panel_auto > 0) {
        if (o.have_keep || o.have_drop || !o.panel_sizes.empty()) { fprintf(stderr, "[E::main] --panel-auto chooses the panel from the reads: not together with --keep-samples, --drop-samples or --panels\n"); return 1; }
        if (!o.cov.empty()) { fprintf(stderr, "[E::main] --panel-auto is not supported together with --coverage\n"); return 1; }
        if (o.devices.size() > 1) { fprintf(stderr, "[E::main] --panel-auto runs on one GPU: not together with --devices of several\n"); return 1; }
    } else if (o.panel_blocks) { fprintf(stderr, "[E::main] --panel-blocks goes with --panel-auto\n"); return 1; }
    if (o.panel_sizes.empty() && o.panel_auto <= 0 && !o.panel_always.empty()) { fprintf(stderr, "[E::main] --panel-always goes with --panels or --panel-auto\n"); return 1; }
    if (!o.panel_sizes.empty()) {
        if (!o.cov.empty()) { fprintf(stderr, "[E::main] --panels is not supported together with --coverage\n"); return 1; }
        if (o.devices.size() > 1) { fprintf(stderr, "[E::main] --panels runs on one GPU: not together with --devices of several\n"); return 1; }
        if (o.panel_sizes.size() > 1)
            for (const std::string &h : o.hap_files)
                if (h.find("{panel}") == std::string::npos) { fprintf(stderr, "[E::main] --panels with several sizes: -o must contain {panel} (got %s), e.g. -o 'out.{panel}.fa'\n", h.c_str()); return 1; }
    }
    if (o.bgzf_index && !o.bgzf) { fprintf(stderr, "[E::main] --bgzf-index goes with --bgzf: the indexes are those of BGZF files\n"); return 1; }
    if (o.calls_files.empty()) {
        if (!o.calls_ref.empty() || !o.calls_contig.empty()) { fprintf(stderr, "[E::main] --calls-ref and --calls-contig go with --calls FILE\n"); return 1; }
        if (o.calls_support) { fprintf(stderr, "[E::main] --calls-support goes with --calls FILE: it adds the read support of every call to that file\n"); return 1; }
    } else {
        if (o.calls_files.size() != o.hap_files.size()) { fprintf(stderr, "[E::main] %zu --calls but %zu -o: one --calls per -o, paired in order (-r a.fq -o a.fa --calls a.vcf -r b.fq -o b.fa --calls b.vcf ...), or none at all\n", o.calls_files.size(), o.hap_files.size()); return 1; }
        if (!o.from_vcf && o.calls_ref.empty()) { fprintf(stderr, "[E::main] --calls with -g needs --calls-ref NAME: the walk the calls are made against, named as the log names walks (SAMPLE.HAP)\n"); return 1; }
        for (const std::string &f : o.calls_files) {
            if (!o.bgzf && f.size() >= 3 && f.compare(f.size() - 3, 3, ".gz") == 0) { fprintf(stderr, "[E::main] --calls %s: without --bgzf the calls are written as plain text (no deflate); give a name that does not end in .gz, or add --bgzf\n", f.c_str()); return 1; }
            if (o.cov.size() > 1 && f.find("{cov}") == std::string::npos) { fprintf(stderr, "[E::main] --coverage with several coverages: --calls must contain {cov} (got %s), e.g. --calls 'out.{cov}x.vcf'\n", f.c_str()); return 1; }
            if (o.panel_sizes.size() > 1 && f.find("{panel}") == std::string::npos) { fprintf(stderr, "[E::main] --panels with several sizes: --calls must contain {panel} (got %s), e.g. --calls 'out.{panel}.vcf'\n", f.c_str()); return 1; }
        }
    }
    o.argc = argc; o.argv = argv;
    t0_real = realtime();

    // The work is done by a child; this process returns the child's status as soon as the child reports it -- after the
    // FASTA is closed and the log written, before the teardown.  Not under a profiler or any other preloaded library that
    // may have started the GPU runtime in this process already (a runtime does not survive a fork), and not when asked.
    bool detach = false;                                      // (opt-in: see the head of this file)
    if (const char *e = getenv("PHI_DETACH")) detach = atoi(e) != 0;
    if (getenv("ROCP_TOOL_LIBRARIES") || getenv("ROCPROFILER_REGISTER_FORCE_LOAD") || getenv("HSA_TOOLS_LIB") || getenv("ROCPROF_OUTPUT_PATH")) detach = false;
    if (const char *pl = getenv("LD_PRELOAD"))
        for (const char *tool : {"rocprof", "roctracer", "roctx", "rocsys", "omnitrace", "rocpd"})
            if (strstr(pl, tool)) detach = false;
    int report_fd = -1;
    if (detach) {
        int pfd[2];
        if (pipe(pfd) == 0) {
            fflush(nullptr);
            const pid_t pid = fork();
            if (pid > 0) {
                close(pfd[1]);
                unsigned char st = 0;
                ssize_t r;
                do r = read(pfd[0], &st, 1); while (r < 0 && errno == EINTR);
                if (r == 1) _exit(st);
                int ws = 0;                                   // the pipe closed without a status: the child died
                while (waitpid(pid, &ws, 0) < 0 && errno == EINTR) {}
                _exit(WIFEXITED(ws) ? WEXITSTATUS(ws) : 128 + (WIFSIGNALED(ws) ? WTERMSIG(ws) : 0));
            } else if (pid == 0) {
                close(pfd[0]);
                report_fd = pfd[1];
                o.detached = true;
                // (the parent's death ends the child: a killed parent takes it along -- and so does the parent's ordinary exit
                //  right after the status arrived: the child is then inside its teardown, which the signal merely cuts short)
                (void)prctl(PR_SET_PDEATHSIG, SIGTERM);
            } else { close(pfd[0]); close(pfd[1]); }           // no fork: one process
        }
    }
    const int status = run(o);
    fflush(nullptr);
    if (report_fd >= 0) {
        const unsigned char st = (unsigned char)status;
        ssize_t r;
        do r = write(report_fd, &st, 1); while (r < 0 && errno == EINTR);
        // nothing more is written: let a pipe that captures the log see its end now, not when the teardown is over
        close(report_fd); close(0); close(1); close(2);
    }
    // the arrays, the contexts and the runtime are given back by the exit itself (PHI_FULL_TEARDOWN=1 frees them one by one first)
    _exit(status);
}
