// device.hpp -- interface of the HIP device stage (device_build.hip, device_classify.hip, device_sssp.hip, device_replay.hip, device_pairs.hip) towards the C-ABI layer.
#pragma once

#include <string>
#include <thread>
#include <cstdint>
#include <vector>

#include "../../include/mtg_engine.h"
#include "host_graph.hpp"

namespace mtg {

struct Device;

int device_count();
// device memory of a call, reserved ahead of it (device_build.hip)
size_t device_call_bytes_estimate(uint64_t V, uint64_t E, uint64_t k);
void device_reserve_async(uint64_t V, uint64_t E, int device_id = -1);  // helper thread: HIP runtime, code objects, one arena chunk (-1: on the default device)
void device_arena_stats(int device_id, uint64_t out[4]);  // bytes in chunks, live bytes, peak of live bytes, chunks taken from the driver so far
void device_arena_reset_peak(int device_id);
void device_reserve_step_work(Device *d);  // MTG_DEVICE_RESERVE_WORK
size_t device_step_work_bytes_estimate(uint64_t V, uint64_t E);
void device_set_default(int device_id);
void device_set_reserve_ahead(int on);  // 0: host-only graph constructors reserve nothing on any GPU
void device_drop_foreign_reservation(const int *used, int n);  // a constructor's provisional chunk on a device the call did not use goes back
int device_get_default();
// lower_bounds: the goal-directed lower bounds (k <= 255) are computed with the graph; without them the search explores full balls
// (same candidate lists) until device_build_lower_bounds adds them
Device *device_create(const HostGraph &g, uint64_t k, int device_id, bool lower_bounds = true);
void device_build_lower_bounds(Device *d, void *stream);
double device_lower_bounds_ms(const Device *d);   // GPU time (HIP events) of that precompute, 0 if the device graph has none
bool device_has_lower_bounds(const Device *d);
void device_free(Device *d);
void device_set_single_use(Device *d);  // the caller searches once: the search's arrays go back before the claim replay (device_pairs.hip)
uint64_t device_graph_bytes(const Device *d);
uint64_t device_classify(Device *d, void *stream);
void device_classify_download(Device *d, void *stream, uint32_t *out_nodes, int32_t *mult, uint8_t *live);
const uint32_t *device_d_out_nodes(const Device *d);
uint64_t device_n_sources(const Device *d);
int device_sssp(Device *d, void *stream, uint64_t src_begin, uint64_t src_end, uint64_t *d_pool, uint64_t pool_cap,
                uint64_t *d_cand_start, uint32_t *d_cand_count, uint64_t *pool_needed);
void device_sssp_count(Device *d, void *stream, uint64_t src_begin, uint64_t src_end, mtg_sssp_stats *stats);
void device_sssp_count_visited(Device *d, void *stream, uint64_t src_begin, uint64_t src_end, mtg_sssp_stats *stats);
bool device_prunes(const Device *d);
uint64_t device_last_active_sources(const Device *d);
double device_last_kernel_ms(const Device *d);
const char *device_last_level_name(const Device *d, int level);
int device_last_levels(const Device *d, double *ms, uint64_t *sources, int cap);
int device_set_plan(Device *d, int plan);
int device_last_replay_rounds(const Device *d);
void device_set_replay_tuning(Device *d, uint64_t windows, int block, int grid, int role_mod, int plain_barrier);
void device_last_replay_ms(const Device *d, double out[2]);
uint64_t device_last_replay_visits(const Device *d);
void device_performance_data(Device *d, void *stream, mtg_dijkstra_performance_data *out);
uint64_t device_replay(Device *d, void *stream, uint64_t n_sources, const uint64_t *d_cand_start, const uint32_t *d_cand_count,
                       const uint64_t *d_pool, mtg_pair **pairs_out, int *rounds_out);
// (pairs_out == nullptr in device_replay / device_pairs / device_pairs_multi: the pairs are not downloaded, they stay in the HBM of the
// (first) device for a finish there)
uint64_t device_pairs(Device *d, void *stream, mtg_pair **pairs_out, int *rounds_out);
int device_id_of(const Device *d);
bool device_matches(const Device *d, const HostGraph &g, uint64_t k);
const mtg_pair *device_resident_pairs(const Device *d, uint64_t *n_out);
mtg_pair *device_take_pairs(Device *d, uint64_t *n_out);
void device_free_array(int device_id, void *p);
uint64_t device_download_pairs(Device *d, mtg_pair **pairs_out);
// SURVEY 8e inside the library: sources block-partitioned by work over the devices, candidate lists gathered on devs[0]
void device_last_pairs_wall_s(const Device *d, double out[3]);  // host wall clock of the last device_pairs[_multi] on d: {SSSP stage (+ gather), claim replay, pair download}
uint64_t device_pairs_multi(Device *const *devs, int n_dev, mtg_pair **pairs_out, int *rounds_out, double *gather_ms_out);
std::vector<uint64_t> device_partition_sources(Device *d, void *stream, int parts);
// euler_device.hip: Euler bicycles on the GPU (valid, but not in the reference's order)
Walks device_euler_cycles(const HostGraph &g, int device_id, double *kernel_ms_out);
void device_euler_force_bitmap(int on);
// finish_device.hip: insertion + Euleriser + Euler bicycles + cut on the GPU (see mtg_finish_device)
// (d_pairs_resident: the n_pairs pairs as they lie in the HBM of `device_id`, e.g. left there by the claim replay -- `pairs` may then be null:
// nothing is uploaded, and the host graph gets its dummy weights from a download that runs beside the GPU stages)
// (times_out: 12 values, see mtg_last_finish_device_times / mtg_last_finish_device_stage_ms)
// (sink: the tigs go straight into a caller's clib.rs output arrays instead of a Walks object -- the host threads that empty the
// download ring write the flattened form, clib.rs:393-407 -- and the returned Walks is empty)
struct TigSink {
    int64_t *edge_out = nullptr;    // [>= kept edges]  +/- unitig id, 0 for a dummy edge (clib.rs:397-398)
    uint64_t *insert_out = nullptr; // [>= kept edges]  0 for an original edge, else the dummy's weight (clib.rs:399-403)
    uint64_t *limits_out = nullptr; // [>= tigs]        exclusive end of tig i (clib.rs:405-406)
    uint64_t n_tigs = 0, n_edges = 0;  // filled by the finish
    // a caller's helper thread that touches the pages of the three arrays (it WRITES zero bytes into them): the finish joins it before
    // its first result write, so that no helper write can land after a result (and then does not touch the arrays itself)
    std::thread *pretoucher = nullptr;
};
// (resident_out: the tigs stay in the HBM of `device_id` -- the returned Walks is empty, *resident_out owns the cutter's output
// arrays; whoever wants them on the host calls download(): a caller that asks for counts, flattens through a sink or spells on the GPU
// never pays for the 0.37-GB copy into pageable memory that a step at 2^27 used to end with)
struct ResidentTigs {
    int device = 0;
    uint32_t *d_edges = nullptr;   // [n_edges] edge ids of the tigs, one after the other
    uint32_t *d_limits = nullptr;  // [n_tigs]  exclusive end of tig i
    uint64_t n_edges = 0, n_tigs = 0;
    ResidentTigs() = default;
    ResidentTigs(const ResidentTigs &) = delete;
    ResidentTigs &operator=(const ResidentTigs &) = delete;
    ~ResidentTigs();
    void download(Walks &w) const;  // through the pinned ring; limits widened to 64 bits on the way
};
Walks device_finish(HostGraph &g, const Pair *pairs, uint64_t n_pairs, uint64_t k, int device_id, int euler_mode, double times_out[12],
                    const mtg_pair *d_pairs_resident = nullptr, TigSink *sink = nullptr, ResidentTigs **resident_out = nullptr);
void device_set_finish_tuning(int records, int flags, long record_delay_us);
void device_release_memory(int device_id);
uint64_t device_memory_held(int device_id);
void device_release_graph_cache(const HostGraph &g);
// synth_device.hip: the G-csr generator on the GPU
HostGraph *device_synth_g_csr(uint64_t n_binodes, uint64_t n_self_mirrors, uint64_t n_unitigs, uint64_t seed, uint64_t k,
                              const uint64_t *thresholds, uint64_t n_thresholds, int max_degree, int device_id);
// spell_device.hip: tig spelling on the GPU (bin.rs:466-606 / 667-818), byte-identical to spell.cpp for ACGT input
uint64_t device_write_walks_text(const HostGraph &g, uint64_t n_walks, const uint64_t *limits, const uint32_t *edges, uint64_t k,
                                 const char *seqs, const uint64_t *seq_off, bool gfa, const char *gfa_header, int device_id,
                                 char **out_buf, double *kernel_ms_out, uint64_t *bytes_out, const struct ResidentTigs *resident = nullptr);
// unitig_links_device.hip: the unitig graph with its links (the file's header and DESIGN.md 26 state the contract). times: host wall
// clock of the uploads and the download, HIP-event time of the link kernels, of the text's scans and of the text kernel, the links,
// the bytes of the text, what the text kernel must move at the least, the arena's peak of live bytes.
struct UnitigGraphTimes {
    double upload_ms = 0, link_ms = 0, text_prepare_ms = 0, text_ms = 0, download_ms = 0;
    uint64_t links = 0, bytes = 0, text_min_bytes = 0, peak_arena_bytes = 0;
};
// link_off[2U + 1] and link_to[links] of the original edges, malloc'd (the caller frees); returns the links
uint64_t device_unitig_links(const HostGraph &g, int device_id, uint64_t **link_off_out, uint32_t **link_to_out, UnitigGraphTimes *times);
// the BCALM2 FASTA (gfa == false) or GFA1 text of the n_unitigs records with their links; kc: null, or the abundance sum of every
// unitig. Returns the bytes; *out_buf is malloc'd (the caller frees)
uint64_t device_write_unitig_graph_text(const HostGraph &g, const char *seqs, const uint64_t *seq_off, uint64_t n_unitigs, uint64_t k,
                                        const uint64_t *kc, bool gfa, int device_id, char **out_buf, UnitigGraphTimes *times);
// unitig_components_device.hip: the connected components of the unitig graph over its links (the file's header and DESIGN.md 27
// state the contract). The arrays of UnitigComponentArrays have one entry per component and are malloc'd (the caller frees).
struct UnitigComponentArrays {
    uint32_t *first_unitig = nullptr, *unitigs = nullptr;
    uint64_t *kmers = nullptr, *abundance = nullptr, *links = nullptr;
    uint32_t *dead_ends = nullptr, *irregular = nullptr;
};
// host wall clock of the uploads and the download, HIP-event time of the label kernels and of the statistics kernel, the components,
// the unitigs, the arena's peak of live bytes; and the label kernels' parts: rep / degree, the unions, flatten + scan + numbers
struct UnitigComponentsTimes {
    double upload_ms = 0, label_ms = 0, stats_ms = 0, download_ms = 0, rep_ms = 0, union_ms = 0, flatten_ms = 0;
    uint64_t components = 0, unitigs = 0, peak_arena_bytes = 0;
};
// kmers[U], kc[U] or null (then the abundance is the k-mers); aggregate: per-wave aggregation of the statistics' atomics (the
// default; off only to measure it). *component_of_out[U] is malloc'd. Returns the components.
uint64_t device_unitig_components(const HostGraph &g, const uint64_t *unitig_kmers, const uint64_t *unitig_kc, int device_id, bool aggregate,
                                  uint32_t **component_of_out, UnitigComponentArrays *out, UnitigComponentsTimes *times);
// unitig_bubbles_device.hip: the bubbles of the unitig graph as variant calls (the file's header and DESIGN.md 38 state the
// contract). arm_off has bubbles + 1 entries, carried arms x n_colors (null without masks), the others one per arm; all malloc'd
// (the caller frees).
struct UnitigBubbleArrays {
    uint64_t *arm_off = nullptr;
    uint32_t *arm_unitig = nullptr;
    uint8_t *arm_strand = nullptr;
    uint32_t *arm_kmers = nullptr;
    uint64_t *arm_abundance = nullptr;
    uint32_t *prefix = nullptr, *suffix = nullptr, *differences = nullptr, *carried = nullptr;
};
// host wall clock of the uploads (with the pack) and the download, HIP-event time of keys + group + number, of the allele kernel and
// of the carrier kernel, the bubbles, the arms, the arena's peak of live bytes
struct UnitigBubblesTimes {
    double upload_ms = 0, group_ms = 0, allele_ms = 0, carrier_ms = 0, download_ms = 0;
    uint64_t bubbles = 0, arms = 0, peak_arena_bytes = 0;
};
// the records data[off[u], off[u + 1]) of the graph's unitigs; unitig_kc[U] or null (then the abundance is the k-mers); kmer_colors:
// null, or one mask per k-mer in window order of the store, with n_colors in 1..64. Returns the bubbles.
uint64_t device_unitig_bubbles(const HostGraph &g, const char *seqs, const uint64_t *seq_off, uint64_t n_unitigs, uint64_t k, uint64_t max_arm_kmers,
                               const uint64_t *unitig_kc, const uint64_t *kmer_colors, uint32_t n_colors, int device_id, UnitigBubbleArrays *out,
                               UnitigBubblesTimes *times);
// fasta_in_device.hip: the plain unitig FASTA route -- graph of the (k-1)-mer overlaps of the unitig ends, joined on the GPU
// (records: data[off[u], off[u + 1]), off[0] = 0). times: host wall clock of upload / download / graph build, HIP-event time of the
// join kernels, and the bytes those kernels must move at the least.
struct FastaJoinTimes {
    double parse_ms = 0, upload_ms = 0, kernel_ms = 0, download_ms = 0, build_ms = 0;
    uint64_t bytes = 0;
};
HostGraph *device_graph_from_sequences(const char *data, const uint64_t *off, uint64_t U, uint64_t k, int device_id, FastaJoinTimes *times);
// fasta_in.cpp: parse a plain unitig FASTA file (.gz inflated) and join it on `device_id` (times->parse_ms: the parse)
HostGraph *read_fasta(const char *path, uint64_t k, int device_id, UnitigStore **store_out, FastaJoinTimes *times);
// fasta_in.cpp: the records of any FASTA file (.gz inflated, multi-line, either case -> upper case) as a sequence store: no graph,
// no length rule. The reader of read_fasta.
UnitigStore *read_fasta_records(const char *path);
// kmer_compare_device.hip: do two sequence sets hold the same canonical k-mers? (the file's header states the contract). times: host
// wall clock of the upload and of the whole call, HIP-event time of the kernels.
struct KmerCompareTimes {
    double upload_ms = 0, pack_ms = 0, insert_a_ms = 0, insert_b_ms = 0, count_ms = 0, total_ms = 0;
};
void device_compare_kmer_sets(const char *seq_a, const uint64_t *off_a, uint64_t n_a, const char *seq_b, const uint64_t *off_b, uint64_t n_b,
                              uint64_t k, int device_id, mtg_kmer_comparison *out, KmerCompareTimes *times);
// kmer_query_device.hip: a k-mer set kept on the device and asked, record by record, which k-mers of other sequences it holds (the
// file's header states the contract). times: host wall clock of the uploads, HIP-event time of the kernels; a build sets the first
// three, a query the last three.
struct KmerQueryTimes {
    double build_upload_ms = 0, build_pack_ms = 0, build_insert_ms = 0, query_upload_ms = 0, query_pack_ms = 0, query_probe_ms = 0;
};
struct KmerIndex;
// locating: the index also keeps the smallest position of every class, the packed bases and the record offsets (device_kmer_index_locate)
// weights: one weight per window of the sequences, in window order; the index also keeps the weight of every class --
// that of its smallest window start -- and answers device_kmer_index_abundance. n must equal the windows.
struct KmerWeights {
    const uint32_t *w;
    uint64_t n;
};
// colors: one 64-bit mask per window, in window order; the index also keeps the mask of every class -- that of its
// smallest window start -- and answers device_kmer_index_colors. n must equal the windows, 1 <= n_colors <= 64.
struct KmerColors {
    const uint64_t *c;
    uint64_t n, n_colors;
};
KmerIndex *device_kmer_index_build(const char *seq, const uint64_t *off, uint64_t n, uint64_t k, int device_id, bool locating,
                                   KmerQueryTimes *times, const KmerWeights *weights = nullptr, const KmerColors *colors = nullptr);
bool device_kmer_index_is_locating(const KmerIndex *ix);
bool device_kmer_index_is_weighted(const KmerIndex *ix);
uint64_t device_kmer_index_n_colors(const KmerIndex *ix);  // 0: not coloured
void device_kmer_index_info(const KmerIndex *ix, mtg_kmer_index_info *out);
void device_kmer_index_query(const KmerIndex *ix, const char *seq, const uint64_t *off, uint64_t n, uint64_t *kmers, uint64_t *valid,
                             uint64_t *found, uint64_t *present_bits, uint64_t *valid_bits, KmerQueryTimes *times);
void device_kmer_index_free(KmerIndex *ix);
// The maximal collinear runs of a query's found windows against a locating index, in ascending query position:
// one entry per run in each array. times: host wall clock of the upload, HIP-event time of the kernels (runs: flag, scan, emit).
struct KmerRuns {
    std::vector<uint64_t> q_record, q_start, kmers, t_record, t_start;
    std::vector<uint8_t> strand;  // 0 = +, 1 = -
};
struct KmerLocateTimes {
    double upload_ms = 0, pack_ms = 0, probe_ms = 0, runs_ms = 0;
};
void device_kmer_index_locate(const KmerIndex *ix, const char *seq, const uint64_t *off, uint64_t n, uint64_t *kmers, uint64_t *valid,
                              uint64_t *found, KmerRuns *runs, KmerLocateTimes *times);
// The walks of a query through the records of a locating index (kmer_walks_device.hpp; include/mtg_engine.h states the
// rule), those with at least min_kmers windows, in ascending query position. fields: nine arrays of n words -- q_record, q_start, q_end,
// kmers, steps, first_step, path_len, path_start, path_end --, steps: (t_record << 1) | strand per step, walk after walk. times: as
// KmerLocateTimes, plus the walk stage (flag, scans, emit, compaction).
struct KmerWalks {
    uint64_t n = 0;
    std::vector<uint64_t> fields, steps;
};
struct KmerThreadTimes {
    double upload_ms = 0, pack_ms = 0, probe_ms = 0, runs_ms = 0, walks_ms = 0;
};
void device_kmer_index_thread(const KmerIndex *ix, const char *seq, const uint64_t *off, uint64_t n, uint64_t min_kmers, uint64_t *kmers,
                              uint64_t *valid, uint64_t *found, KmerWalks *walks, KmerThreadTimes *times);
// The query plus, per record over its found windows, the sum, the smallest and the largest weight of their classes (all 0 where
// nothing is found) and, if per_window is given ([off[n]]), the weight at every found window's global start position, 0 elsewhere.
// times: host wall clock of the upload and the download, HIP-event time of the kernels.
struct KmerAbundanceTimes {
    double upload_ms = 0, pack_ms = 0, probe_ms = 0, download_ms = 0;
};
void device_kmer_index_abundance(const KmerIndex *ix, const char *seq, const uint64_t *off, uint64_t n, uint64_t *kmers, uint64_t *valid,
                                 uint64_t *found, uint64_t *sum, uint32_t *min, uint32_t *max, uint32_t *per_window, KmerAbundanceTimes *times);
// The query plus per_color ([n * n_colors], row-major): the found windows of record r whose class's mask has bit c; per_window, if
// given ([off[n]]): the mask at every found window's global start position, 0 elsewhere. stats_ms belongs to the coloured compaction.
struct KmerColorTimes {
    double stats_ms = 0, upload_ms = 0, pack_ms = 0, probe_ms = 0, download_ms = 0;
};
void device_kmer_index_colors(const KmerIndex *ix, const char *seq, const uint64_t *off, uint64_t n, uint64_t *kmers, uint64_t *valid,
                              uint64_t *found, uint32_t *per_color, uint64_t *per_window, KmerColorTimes *times);
// A tally over one index: one 64-bit counter per table slot, zero at creation, from the device arena of the index's
// device until device_kmer_tally_free; the index must outlive it and is not changed. add: the query plus, per found window, one
// more on the counter of its class. coverage: the query plus, per record over its found windows, those whose class has a count > 0,
// the sum of the counts and the largest; per_window, if given ([off[n]]): the count at every found window's global start, 0 elsewhere.
struct KmerTally;
struct KmerTallyTimes {
    double upload_ms = 0, pack_ms = 0, probe_ms = 0, download_ms = 0;
};
KmerTally *device_kmer_tally_create(const KmerIndex *ix);
uint64_t device_kmer_tally_device_bytes(const KmerTally *t);
void device_kmer_tally_add(KmerTally *t, const char *seq, const uint64_t *off, uint64_t n, uint64_t *kmers, uint64_t *valid, uint64_t *found,
                           KmerTallyTimes *times);
void device_kmer_tally_coverage(const KmerTally *t, const char *seq, const uint64_t *off, uint64_t n, uint64_t *kmers, uint64_t *valid,
                                uint64_t *found, uint64_t *covered, uint64_t *sum, uint64_t *max, uint64_t *per_window, KmerTallyTimes *times);
void device_kmer_tally_reset(KmerTally *t);
void device_kmer_tally_free(KmerTally *t);
// Read correction against the index's k-mers (kmer_correct_device.hpp; include/mtg_engine.h states the rule). The query's
// kmers / valid / found on the input, found_after on the corrected text, and per record the candidates of round 1, the ambiguous
// positions of the last round and the positions substituted. *out: the substitutions by ascending global position (bases as the
// letters ACGT), the counts per round, and the phases -- host wall clock of upload, download and the whole call, HIP-event time of
// the kernels. The index is not changed and the call keeps no device memory.
struct KmerCorrectCall {
    std::vector<uint64_t> positions;
    std::vector<uint8_t> bases;
    uint64_t round_corrected[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t candidates = 0;  // of round 1, over all records
    double upload_ms = 0, pack_ms = 0, query_ms = 0, flag_ms = 0, evaluate_ms = 0, apply_ms = 0, download_ms = 0, total_ms = 0;
};
void device_kmer_index_correct(const KmerIndex *ix, uint32_t min_solid, uint32_t rounds, const char *seq, const uint64_t *off, uint64_t n,
                               uint64_t *kmers, uint64_t *valid, uint64_t *found, uint64_t *found_after, uint64_t *candidates, uint64_t *ambiguous,
                               uint64_t *corrected, KmerCorrectCall *out);
// tig_index_device.hip: the sparse minimizer index over a sequence set (the file's header and DESIGN.md 28 state the contract): the
// packed bases plus one word per anchor, asked what device_kmer_index_query is asked. m = 0: tig_index_default_m(k); bucket_limit
// = 0: 64. times: host wall clock of the uploads, HIP-event time of the kernels; a build sets the first five, a query the last three.
struct TigIndexTimes {
    double build_upload_ms = 0, build_pack_ms = 0, build_anchors_ms = 0, build_directory_ms = 0, build_heavy_ms = 0, query_upload_ms = 0,
           query_pack_ms = 0, query_probe_ms = 0;
};
struct TigIndex;
uint64_t tig_index_default_m(uint64_t k);  // min(19, ceil(2 k / 3))
TigIndex *device_tig_index_build(const char *seq, const uint64_t *off, uint64_t n, uint64_t k, uint64_t m, uint64_t bucket_limit, int device_id,
                                 TigIndexTimes *times, bool locating = false, const char *fn = nullptr);
void device_tig_index_info(const TigIndex *ix, mtg_tig_index_info *out);
// locating: the index also keeps the smallest window start of every class of its heavy buckets (8 B per table slot) and
// answers device_tig_index_locate: device_kmer_index_locate's contract and results, at the coordinates of the sequences it was built from.
bool device_tig_index_is_locating(const TigIndex *ix);
void device_tig_index_locate(const TigIndex *ix, const char *seq, const uint64_t *off, uint64_t n, uint64_t *kmers, uint64_t *valid,
                             uint64_t *found, KmerRuns *runs, KmerLocateTimes *times);
void device_tig_index_thread(const TigIndex *ix, const char *seq, const uint64_t *off, uint64_t n, uint64_t min_kmers, uint64_t *kmers,
                             uint64_t *valid, uint64_t *found, KmerWalks *walks, KmerThreadTimes *times);  // device_kmer_index_thread's contract
void device_tig_index_query(const TigIndex *ix, const char *seq, const uint64_t *off, uint64_t n, uint64_t *kmers, uint64_t *valid,
                            uint64_t *found, uint64_t *present_bits, uint64_t *valid_bits, TigIndexTimes *times);
// payloads by position (tig_payload_device.hpp): a locating index that also keeps one weight and / or one colour mask
// per window of its sequences (KmerWeights / KmerColors as device_kmer_index_build takes them; layout 0: each payload takes the
// smaller of dense and runs, 1: dense, 2: runs) and answers device_kmer_index_abundance's / _colors' contracts with their results.
// times: build {upload, reduce, flag + scan, compact or narrow} per payload; call {upload, pack, probe, gather}.
struct TigPayloadTimes {
    double weights_ms[4] = {0, 0, 0, 0}, colors_ms[4] = {0, 0, 0, 0};
    double upload_ms = 0, pack_ms = 0, probe_ms = 0, gather_ms = 0;
};
TigIndex *device_tig_index_build_annotated(const char *seq, const uint64_t *off, uint64_t n, uint64_t k, uint64_t m, uint64_t bucket_limit,
                                           const KmerWeights *weights, const KmerColors *colors, int layout, int device_id, TigIndexTimes *times,
                                           TigPayloadTimes *payload_times);
void device_tig_index_payload_info(const TigIndex *ix, mtg_tig_payload_info *out);
void device_tig_index_abundance(const TigIndex *ix, const char *seq, const uint64_t *off, uint64_t n, uint64_t *kmers, uint64_t *valid,
                                uint64_t *found, uint64_t *sum, uint32_t *min, uint32_t *max, uint32_t *per_window, TigPayloadTimes *times);
void device_tig_index_colors(const TigIndex *ix, const char *seq, const uint64_t *off, uint64_t n, uint64_t *kmers, uint64_t *valid,
                             uint64_t *found, uint32_t *per_color, uint64_t *per_window, TigPayloadTimes *times);
void device_tig_index_free(TigIndex *ix);
// the index as a file (tig_index_file_device.hpp). save: false and err = why the file could not be written. load: null
// and err = "<path>: <section>: <check>" for a file that is refused, with every allocation returned; meta: the file's metadata blob.
// times: of a save {digest kernels, download, write}, of a load {read, upload, digest kernels, validation kernel}, in ms.
struct TigIndexFileTimes {
    double save_digest_ms = 0, save_download_ms = 0, save_write_ms = 0, load_read_ms = 0, load_upload_ms = 0, load_digest_ms = 0, load_validate_ms = 0;
};
bool device_tig_index_save(const TigIndex *ix, const char *path, const char *meta, uint64_t meta_len, TigIndexFileTimes *times, std::string &err);
TigIndex *device_tig_index_load(const char *path, int device_id, std::string &meta, TigIndexFileTimes *times, std::string &err);
// A tally over one locating sparse index (tig_tally_device.hpp): device_kmer_tally_*'s contracts and results with one
// 64-bit counter per window ordinal of the indexed text (plus win_off[records + 1] where the index keeps none), counted at the first
// occurrence of a window's class. counters: the W counters in window order. times: host wall clock of the upload and the download,
// HIP-event time of the kernels; pass2: the add or the gather.
struct TigTally;
struct TigTallyTimes {
    double upload_ms = 0, pack_ms = 0, probe_ms = 0, pass2_ms = 0, download_ms = 0;
};
TigTally *device_tig_tally_create(const TigIndex *ix);
uint64_t device_tig_tally_device_bytes(const TigTally *t);
uint64_t device_tig_tally_windows(const TigTally *t);
void device_tig_tally_add(TigTally *t, const char *seq, const uint64_t *off, uint64_t n, uint64_t *kmers, uint64_t *valid, uint64_t *found,
                          TigTallyTimes *times);
void device_tig_tally_coverage(const TigTally *t, const char *seq, const uint64_t *off, uint64_t n, uint64_t *kmers, uint64_t *valid,
                               uint64_t *found, uint64_t *covered, uint64_t *sum, uint64_t *max, uint64_t *per_window, TigTallyTimes *times);
void device_tig_tally_counters(const TigTally *t, uint64_t *out);
void device_tig_tally_reset(TigTally *t);
void device_tig_tally_free(TigTally *t);
// Pseudoalignment on a coloured index of either kind (pseudoalign_device.hpp; include/mtg_engine.h states the rule).
// A fragment is record r of the reads or, with mates (both pointers given, the same n), the pair of record r of each: kmers, valid and
// found are the query's columns summed over its records, masks[f] the colours the rule assigns. base: the ordinal of fragment 0.
// *out: the call's equivalence classes in no particular order, its totals, and the phases -- host wall clock of the uploads and the
// download, HIP-event time of the kernels (probe: every colour probe of the call).
struct PseudoalignRule {
    uint64_t permille, min_kmers;
    uint32_t over_valid;  // the denominator: 0 found, 1 valid
};
struct PseudoalignCall {
    std::vector<uint64_t> mask, fragments, first;
    uint64_t eligible = 0, assigned = 0, ambiguous = 0;
    double upload_ms = 0, pack_ms = 0, probe_ms = 0, mask_ms = 0, dictionary_ms = 0, download_ms = 0;
};
void device_kmer_index_pseudoalign(const KmerIndex *ix, const PseudoalignRule &rule, uint64_t base, const char *seq, const uint64_t *off, uint64_t n,
                                   const char *mate_seq, const uint64_t *mate_off, uint64_t *kmers, uint64_t *valid, uint64_t *found, uint64_t *masks,
                                   PseudoalignCall *out);
uint64_t device_tig_index_n_colors(const TigIndex *ix);  // 0: not coloured
void device_tig_index_pseudoalign(const TigIndex *ix, const PseudoalignRule &rule, uint64_t base, const char *seq, const uint64_t *off, uint64_t n,
                                  const char *mate_seq, const uint64_t *mate_off, uint64_t *kmers, uint64_t *valid, uint64_t *found, uint64_t *masks,
                                  PseudoalignCall *out);
// compact_device.hip: the maximal unitigs of the k-mer set of arbitrary sequences (the file's header and DESIGN.md 16 state the
// contract), as an ordinary sequence store. times: host wall clock of upload, download and the whole call, HIP-event time of the
// kernel phases, the pointer-jumping rounds, the bytes the kernels must move at the least, the arena's peak of live bytes.
struct CompactTimes {
    double upload_ms = 0, pack_ms = 0, insert_ms = 0, ids_ms = 0, nodes_ms = 0, rank_ms = 0, emit_ms = 0, download_ms = 0, total_ms = 0;
    int rounds = 0;
    uint64_t bytes = 0, peak_arena_bytes = 0;
    double filter_ms = 0, select_ms = 0;  // selected calls: the filter probe (ids_ms leaves it out), the keep kernel and the move
};
// What a counted call adds: the k-mers whose abundance reaches m, the statistics of the counting and, per unitig in the
// store's order, the sum of its k-mers' abundances. The spectrum sweep is booked under ids_ms, the sums under emit_ms.
struct Counted {
    uint64_t m;
    mtg_abundance *abundance;
    std::vector<uint64_t> *sums;
    // null, or: every kept k-mer's abundance in window order of the output store -- entry (windows of the earlier
    // unitigs) + j belongs to the k-mer at offset j of unitig u --, the array the sums are scanned from; its download is booked
    // under download_ms
    std::vector<uint32_t> *kmer_counts;
};
// What a coloured call adds to a counted one that hands out the counts: a colour per record in, every kept k-mer's
// colour mask (indexed like kmer_counts) and the statistics over the masks out.
struct Colored {
    const uint8_t *record_colors;  // [n_rec], each < n_colors
    uint64_t n_colors;
    std::vector<uint64_t> *kmer_colors;
    mtg_color_stats *stats;
    double *stats_ms;  // HIP-event time of color_stats_kernel (part of emit_ms)
};
// What a call with colour classes adds to a coloured one: the distinct masks of the output store numbered in the order
// of the first window that shows them; per class its mask, k-mers, runs (maximal stretches of consecutive windows of one unitig with
// equal masks) and first window; per window its class. times: HIP-event time of the dictionary's phases, its download by the host clock.
struct ColorClasses {
    std::vector<uint64_t> masks, kmers, runs, first;
    std::vector<uint32_t> kmer_class;
    uint64_t n_runs = 0;
};
struct ColorClassTimes {
    double heads_ms = 0, table_ms = 0, ids_ms = 0, counts_ms = 0, download_ms = 0;
};
struct Classed {
    bool split;  // a node is passable only if the k-mers that enter and leave it have equal masks: every unitig is one run
    ColorClasses *out;
    ColorClassTimes *times;
};
// What a cleaned call adds: tip clipping and the removal of isolated unitigs in rounds before the final pass. It
// needs no rung below it; removed_occurrences is 0 unless the call is counted. clean_ms: HIP-event time of the decision and removal
// kernels over all rounds.
struct Cleaned {
    mtg_cleaning_params params;
    mtg_cleaning *out;
    double *clean_ms;
};
// What a simplified call adds to a cleaned one: the rounds also pop the weaker arms of simple bubbles. It goes with a
// Cleaned (whose params carry the rounds) and, where max_arm_kmers > 0, with a Counted. bubble_ms: HIP-event time of the list, sums,
// choose and verdict kernels over all rounds, which clean_ms leaves out.
struct Bubbled {
    mtg_bubble_params params;
    mtg_bubbles *out;
    double *bubble_ms;
};
// What a selected call adds (include/mtg_engine.h states the rules): of S_m only the k-mers that pass the colour rules
// and the rules against the filter records -- a second store (data, off, n_rec, one role byte per record: 0 subtract, 1 intersect)
// that is probed in the k-mer table while it lives and never inserted -- reach nodes, succ and everything behind them. It stands
// beside the ladder like Cleaned, needs a Counted (m may be 1) and, if a colour rule is set, a Colored, whose statistics are then
// taken over S_m. The probe is booked under CompactTimes::filter_ms, the keep kernel with its scan and move under select_ms.
struct Selected {
    mtg_selection_params params;
    const char *filter_data;
    const uint64_t *filter_off;
    const uint8_t *filter_roles;
    uint64_t filter_n;
    mtg_selection *out;
};
// One compaction. who: the public entry point that was called, for the messages. Each rung of the ladder is one pointer, null where
// the call does not climb that far; a rung needs the ones below it.
struct CompactRequest {
    const char *who;
    const char *data;
    const uint64_t *off;
    uint64_t n_rec, k;
    int device_id;
    mtg_compaction *stats_out;
    CompactTimes *times;
    const Counted *counted;
    const Colored *colored;
    const Classed *classed;
    const Cleaned *cleaned = nullptr;
    const Bubbled *bubbles = nullptr;
    const Selected *selected = nullptr;
};
UnitigStore *device_compact_unitigs(const CompactRequest &rq);
// ... of masks and unitig lengths handed in (kmer_colors: n masks in window order, none 0; unitig_kmers: n_unitigs lengths that sum to n)
void device_color_classes(const uint64_t *kmer_colors, uint64_t n, const uint64_t *unitig_kmers, uint64_t n_unitigs, int device_id, ColorClasses *out,
                          ColorClassTimes *times);
// the counts kernel's LDS table (classes), largest grid and block: what a test must exceed to reach the kernel's other paths
uint64_t device_color_class_limit(int which);
// fasta_in.cpp: read_fasta_records without an alphabet rule and without case folding (the queries of the k-mer index), plus the
// record names (the header text behind `>` up to the first white space) as a second store
UnitigStore *read_fasta_records_named(const char *path, UnitigStore **names_out);
// fasta_in.cpp: read_fasta_records where a run of characters outside ACGT ends a piece instead of aborting; empty pieces are dropped
UnitigStore *read_fasta_records_split(const char *path, uint64_t *pieces_cut);
// fastq_device.hip: FASTQ reads read on the GPU (the file's header and DESIGN.md 21 state the contract). named: the records whole
// plus their names, else the pieces of good bases. Returns 0, or 1 with the message of a malformed file in err and no store.
// times: host wall clock of read + inflate, upload, download and the whole call, HIP-event time of the kernel phases.
struct FastqTimes {
    double read_ms = 0, upload_ms = 0, lines_ms = 0, pieces_ms = 0, download_ms = 0, total_ms = 0;
};
int device_read_fastq(const char *path, uint64_t min_base_quality, int device_id, bool named, UnitigStore **seqs_out, UnitigStore **names_out,
                      mtg_fastq_stats *stats_out, FastqTimes *times, char *err, uint64_t err_capacity);
void device_candidates_to_host(Device *d, void *stream, std::vector<uint64_t> &cand_start,
                               std::vector<uint32_t> &cand_count, std::vector<uint64_t> &pool);

}  // namespace mtg
