// options.h — the command-line surface of `pandepth` (-i -o -g -f -b -w -a -q -d -x -t -s -c -r -h; of its own: -dist -levels -quantile -thresholds -gcbias -del -frag -fragmax -readstats -rowreads -alnstats);
// -i takes SAM / BAM / CRAM 2.1 / 3.0 / 3.1 / PAF files or a #.list of them.
// Behaviour follows the reference's parser (PD:84-293) including its quirks: every '-' is
// stripped from a flag, `*.list`/`*.List` expands to one input per non-empty line, -w < 1 and
// -d < 1 clamp to 1, -o gets ".gz" appended and a trailing ".stat"/".bed" dropped later.
#ifndef PD_OPTIONS_H_
#define PD_OPTIONS_H_
#include <stdint.h>
#include <string>
#include <vector>

namespace pdh {

struct Options {
    std::vector<std::string> inputs;     // InStr1List
    std::string input;                   // InStr1
    std::string region_file;             // InStr2 (gff/gtf or bed)
    std::string out;                     // InStr3 (with ".gz")
    std::string feature = "CDS";
    int mode = 0;                        // InInt2: 0 chr, 1 gff, 2 gtf, 3 bed3, 4 bed4, 5 window >= 150, 6 window < 150
    int min_mapq = -1;                   // main() presets -1 (PD:3444): nothing is filtered unless -q is given
    int min_dep = 1;
    uint32_t flag_mask = 1796;
    int threads = 3;
    int decode_readers = 0;                                // device decode: reader threads per context (0: min(threads, 6)); a `#.list` run sets it so that a context's readers do not shrink with -t / #GPUs — they wait for the device most of the time
    std::string reference;            // -r: FASTA behind -c's GC(%) column (host/fasta.h)
    int win = 0;
    bool site_out = false;               // -a
    bool use_index = true;               // hidden -s clears it
    bool gc = false;
    int dist = 0;                        // -dist N (not in the reference): <out>.dist.stat.gz, depths 0 .. N-1 and >= N per contig
    bool levels = false;                 // -levels SPEC (not in the reference): <out>.levels.bed.gz, runs of equal depth ('exact': levels_edges empty) or depth class
    std::vector<uint32_t> levels_edges;  // the classes' lower edges, strictly ascending, at most 64
    std::vector<uint32_t> quantile;      // -quantile SPEC (not in the reference): <out>.quantile.stat.gz, per-row depth percentiles; 1..16 values in 0..100, strictly ascending
    bool count_del = false;              // -del (not in the reference): deletions count as covered — one run per group of M/=/X/D operations that no N splits, instead of one per M/=/X
    bool frag = false;                   // -frag (not in the reference): a properly paired read with tlen > 0 counts as the one run [pos, pos + tlen), its mate as nothing; clears use_index
    uint32_t frag_max = 0x7FFFFFFFu;     // -fragmax N, 1 .. 2^31 - 1 (needs -frag): pairs with |tlen| above it are two ordinary reads
    uint32_t gcbias = 0;                 // -gcbias W (not in the reference; needs -r): <out>.gcbias.stat.gz, depth by GC content of windows of W cells, 1 .. 2^20 (0: off)
    uint32_t readstats = 0;              // -readstats N (not in the reference): <out>.reads.stat.gz, what the records were — classes, flag bits, per contig, MAPQ, insert sizes 1 .. N-1 and >= N; 1 .. 65536 (0: off)
    uint32_t alnstats = 0;               // -alnstats W (not in the reference): <out>.aln.stat.gz, the CIGAR operations, indel lengths, read lengths (N50) and aligned fractions of the records, in length bins of W bases; 1 .. 65536 (0: off)
    bool rowreads = false;               // -rowreads (not in the reference): <out>.rowreads.stat.gz, the records that start in every row of the main table — counts by filter class, strand, mean MAPQ
    std::vector<uint32_t> thresholds;    // -thresholds SPEC (not in the reference): <out>.thresholds.stat.gz, per-row counts of cells at or above each depth; 1..16 values below 2^31, strictly ascending
};

// Returns the number of input files (0 => nothing to do / message already printed), like
// bamCov_help01.  Messages go to stdout/stderr exactly as the reference prints them.
int parse_options(int argc, char **argv, Options *o);
void print_help();

// Development switches of the executable — which of its equivalent paths runs (device or host decode, where the gzip streams are
// parsed, how many decode threads / GPUs ...), never what it prints — come in through ONE door: the hidden option `-X key=value[,key=value]`
// or the environment variable PANDEPTH_TUNE with the same syntax (tests, benchmarks).  tune("key") returns the value or NULL.
//   device_decode=0  device_deflate=0  site_resident=0  table_resident=0  table_resident_min=N  site_overlap=0  site_identical=0|1
//   site_parallel_min=N  pgz_min=N  rccl=0|force  rccl_verbose=1  gpus=N  dd_threads=N  dd_depth=N  dd_batch_mb=N  inflate_waves=N  lz_group=N  decode_only=1
//   decode_fast=0 (the host confirms every batch's record chain, as before round 5)  decode_max_redo=N  decode_spoil=K (test hook: plants wrong guesses)
//   round 6: transport=peer|rccl (the list mode's collective: in-process peer copies — the default — or RCCL made ahead of the contexts)
//   comm=0|force (no communicator / one even for a single context; `rccl=0|force` are the same switches under their older names)
//   comm_early=0 (the communicator and its buffers in line before the first collective instead of beside the decode)
//   h2d_kernel=1|2|3 (a batch's bytes fetched by a copy kernel / + its tables / read in place by the inflate kernel: all measured slower)
//   h2d_fifo=0 (every batch's copy on its own stream, as until round 6; default: first come, first served on the main stream, one copy per batch)
//   sync_event=0 (collect waits for the batch's stream instead of its last event)  h2d_lanes=2 (two copies on the link at a time)
//   dd_trace=1 (with PANDEPTH_TIMING: a [trace] line per batch, tools/feeder_trace.py)  dd_inflight=N (at most N batches queued at a time)
//   dd_pin_ahead=N (buffers page-locked before the readers start)  decode_warm=1 (the slots made ready by a helper thread)  lz_calls=4 (provider calls of a gzip round in flight)
//   levels_chunk=N (cells per pd_depth_levels call of the -levels writer; default 2^24)
//   quantile_wave_max=N  quantile_split_cells=N (pd_set_param keys of the -quantile kernels: the row sizes at which the launch shape changes, see pandepth_amd_dev.h)
//   quantile_device=0 (the -quantile rows selected on the host threads from cells read back, as an engine without the entry points does)
//   threshold_wave_max=N (pd_set_param key of the -thresholds kernels: the row size above which a row is counted in pieces, see pandepth_amd_dev.h)
//   thresholds_device=0 (the -thresholds rows counted on the host threads from cells read back, as an engine without the entry points does)
//   gcbias_piece_cells=N  gcbias_wave_max=N (pd_set_param keys of the -gcbias pass: the piece size and the width at which the launch shape changes, see pandepth_amd_dev.h)
//   gcbias_device=0 (the -gcbias windows binned on the host threads from cells read back, as an engine without the entry point does)
//   environment: PANDEPTH_DEVTRACE=1 (a [devtrace] line per batch: host-clock times of its stage events; first batches: what pd_decode_queue's own time went to)
// -X is not part of the reference's command line (which answers an unknown flag with "Error UnKnow argument"): it is accepted only in this
// spelling, is not listed by -h, and a PANDEPTH_* variable of the earlier rounds that is still set gets a note on stderr.
const char *tune(const char *key);
long long tune_int(const char *key, long long dflt);
void tune_add(const std::string &kv_list);

// text-file helper shared with the region parser: whole file (plain or gzip) split into lines
// the way `while(!in.eof()) getline(in, line)` sees them
bool read_lines(const std::string &path, std::vector<std::string> *lines);

} // namespace pdh
#endif
