/*
 * mtg_engine.h -- engine-level C-ABI underneath matchtigs.h (NEW; the reference has no such layer).
 *
 * It is what both the clib.rs-compatible shim (matchtigs_compute_tigs) and a Rust
 * `impl TigAlgorithm for GreedytigAlgorithm` body (src/implementation/greedytigs/mod.rs:75-90,
 * see INTEGRATION.md) call: an edge-centric bigraph in, (out,in,distance) pairs and tig walks out.
 * Stages are exported separately so that they can be parity-checked tier by tier and so that
 * bench.py / a multi-GPU driver can shard the SSSP stage across ranks:
 *
 *   stage                          reference lines it replaces                      where it runs
 *   mtg_classify                   greedytigs/mod.rs:222-255 (eulertigs :64-97)     GPU (HIP)
 *   mtg_sssp_candidates            greedytigs/mod.rs:324-335 + traitgraph-algo      GPU (HIP)
 *                                  Dijkstra::shortest_path_lens (all sources at once)
 *   mtg_replay_claims_device       greedytigs/mod.rs:301-523 (1-thread order)       GPU (HIP)
 *   mtg_replay_claims              the same loop over host arrays (A/B, tests)      host (C++)
 *   mtg_finish_greedytigs          greedytigs/mod.rs:678-801 + implementation/      host (C++); Euler bicycles optionally
 *                                  mod.rs:392-649 + bigraph Euler decomposition     on the GPU (mtg_config.euler_mode)
 *   mtg_compute_eulertigs          eulertigs/mod.rs:48-198                          host (C++); idem
 *   mtg_write_walks_fasta / _gfa   bin.rs:466-606 / 667-818                         host (C++)
 *   mtg_read_bcalm2                bin.rs:902-912 (genome-graph bcalm2 reader)      host (C++)
 *   mtg_read_fasta                 bin.rs:891-901 (genome-graph fasta reader)       GPU (HIP) join, host (C++) parse
 *
 * All pointers are plain host pointers unless the name starts with d_ (device pointer in the
 * HBM of the GPU the mtg_device was created on). `stream` is a hipStream_t passed as void*
 * (NULL = the default stream). No torch types anywhere.
 *
 * Errors follow the reference's convention (panic => abort): message on stderr + abort().
 * Functions that can fail recoverably return a status code instead, documented per function.
 */
#ifndef MTG_ENGINE_H
#define MTG_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mtg_graph mtg_graph;   /* host bigraph; grows when dummy edges are inserted */
typedef struct mtg_device mtg_device; /* one GPU: device-resident graph + workspaces */
typedef struct mtg_walks mtg_walks;   /* a list of edge walks (tigs or Euler cycles) */

/* (out_node, in_node, distance): one matched pair, greedytigs/mod.rs:461. */
typedef struct {
    uint32_t out_node;
    uint32_t in_node;
    uint64_t distance;
} mtg_pair;

/* Counters of one SSSP stage (SURVEY.md 8d "unit of work"). */
typedef struct {
    uint64_t sources;          /* sources processed */
    uint64_t settled_nodes;    /* (source,node) pairs with distance <= k-1 (full ball) */
    uint64_t relaxed_edges;    /* sum of out-degrees of settled nodes = SSSP edges */
    uint64_t emitted;          /* candidates written */
    uint64_t relax_attempts;   /* edge relaxations the label-correcting kernel really performed */
    uint64_t overflow_sources; /* sources that needed a larger kernel level */
} mtg_sssp_stats;

/* Engine configuration = the fields of GreedytigAlgorithmConfiguration (greedytigs/mod.rs:40-73; the C-ABI fixes
 * them at clib.rs:378-389, the CLI fills them from bin.rs:1074-1082) plus what only this engine has.
 * threads / staged_parallelism_divisor / resource_limit_factor / node_weight_array_type / heap_type select CPU data
 * structures and scheduling in the reference and never change its 1-thread result; the engine validates and otherwise
 * ignores them (results always equal the reference's 1-thread order, its only deterministic one). */
enum { MTG_NODE_WEIGHT_EPOCH_ARRAY = 0, MTG_NODE_WEIGHT_HASHBROWN_HASH_MAP = 1 }; /* implementation/mod.rs:61-81 */
enum { MTG_HEAP_STD_BINARY_HEAP = 0 };                                            /* implementation/mod.rs:83-102 */
enum { MTG_PERFORMANCE_DATA_NONE = 0, MTG_PERFORMANCE_DATA_COMPLETE = 1 };        /* implementation/mod.rs:104-126 */
enum { MTG_EULER_HOST_REFERENCE_ORDER = 0, MTG_EULER_DEVICE = 1 };
/* Where dummy insertion, the Euleriser and the cutter run: AUTO = on the GPU (device_ids[0]) whenever one is visible and the
 * graph holds only its original edges, else the host stages; HOST / DEVICE force one (DEVICE aborts without a GPU). Both give
 * the same edges and tigs: the GPU Euleriser reproduces the reference's sequence of breaking edges. With
 * MTG_EULER_HOST_REFERENCE_ORDER the device stage builds the walk's node records and the host only walks. */
enum { MTG_FINISH_AUTO = 0, MTG_FINISH_HOST = 1, MTG_FINISH_DEVICE = 2 };
#define MTG_MAX_DEVICES 8
typedef struct {
    uint64_t struct_size;              /* sizeof(mtg_config) of the header the caller was built against: set by mtg_config_init and checked by
                                          every function that takes a configuration. ALWAYS fill a configuration through mtg_config_init.
                                          New fields are only ever APPENDED: a caller built against an older header (struct_size smaller,
                                          down to MTG_CONFIG_MIN_SIZE = the layout of round 4) keeps working -- the fields it does not
                                          know take the values mtg_config_init gives them --, a struct_size LARGER than this library's
                                          (a caller newer than the library) or below the minimum aborts with a message. */
    uint64_t threads;                  /* greedytigs/mod.rs:42 */
    uint64_t k;                        /* :44 */
    double staged_parallelism_divisor; /* :47, 0 = None */
    uint64_t resource_limit_factor;    /* :49 */
    int32_t node_weight_array_type;    /* :51 */
    int32_t heap_type;                 /* :53 */
    int32_t performance_data_type;     /* :55; COMPLETE additionally runs the counting kernels (mtg_last_performance_data) */
    int32_t euler_mode;                /* MTG_EULER_HOST_REFERENCE_ORDER (bit-exact tigs) or MTG_EULER_DEVICE (valid walks, same
                                          #tigs / cumulative length, different order) */
    int32_t n_devices;                 /* GPUs to shard the SSSP sources over; >= 1 */
    int32_t device_ids[MTG_MAX_DEVICES];
    /* MatchtigAlgorithmConfiguration (matchtigs/mod.rs:33-45), tig algorithm 4 only; may be NULL otherwise */
    const char *matching_file_prefix; /* the instance goes to <prefix>.minimalperfectmatching, the matcher writes <that>.solution */
    const char *matcher_path;         /* blossom5-compatible executable: `<matcher> -e <instance> -w <solution>` */
    int32_t finish_stage;              /* MTG_FINISH_AUTO / _HOST / _DEVICE (appended in round 3) */
    int32_t reserved0;
} mtg_config;
#define MTG_CONFIG_MIN_SIZE 120 /* sizeof(mtg_config) of round 4, the oldest layout with struct_size in front */
/* GreedytigAlgorithmConfiguration::new(threads, k) (greedytigs/mod.rs:62-72): staged None, factor 0, HashbrownHashMap,
 * StdBinaryHeap, performance data None; engine fields: host Euler walk, one device (id 0). */
void mtg_config_init(mtg_config *cfg, uint64_t threads, uint64_t k);

/* The reference's Dijkstra performance counters (logged at greedytigs/mod.rs:647-673; DijkstraPerformanceData of
 * traitgraph-algo) in the engine's terms, over all queries of the last greedy run with performance_data_type COMPLETE.
 * The engine searches the FULL (k-1)-ball of every source with a label-correcting wavefront, one source per workgroup in
 * this mode: iterations = expansions of a settled (source,node) pair; heap pushes = frontier-log items; unnecessary heap
 * elements = log items superseded by a shorter distance before they were expanded (the analogue of a stale heap entry);
 * max heap size of a query = its frontier-log length; max distance array size of a query = its table entries. */
typedef struct {
    uint64_t dijkstras;                 /* number of queries */
    uint64_t iterations;
    uint64_t heap_pushes;
    uint64_t unnecessary_heap_elements;
    uint64_t max_max_heap_size;
    uint64_t max_max_distance_array_size;
    uint64_t sum_max_heap_size;           /* average_max_heap_size = sum / dijkstras */
    uint64_t sum_max_distance_array_size; /* average_max_distance_array_size = sum / dijkstras */
} mtg_dijkstra_performance_data;

/* Library / device probes. */
const char *mtg_version(void);
int mtg_device_count(void); /* hipGetDeviceCount; 0 when no GPU (never initialises a context) */
/* Which setting of the four out-of-tree policies (include/mtg_policy.h: heap tie-break, inclusive bound, adjacency order, union-find
 * tie) this library was built with: bit i set = policy P(i+1) flipped. 0 for libmatchtigs.so; 15 for the libmatchtigs_flipped.so
 * that `make flipped` builds for the parity suite. */
unsigned mtg_policies(void);

/* ---- host graph ------------------------------------------------------------------------ */
/* Edges in id order: edge 2u = unitig u forwards, edge 2u+1 = its mirror (clib.rs:239-248).
 * weight = k-mers of the unitig (bin.rs:357-379). Validates node pairing and the edge mirror
 * property like clib.rs:251-252 (abort on violation). Arrays are copied. */
mtg_graph *mtg_graph_from_edges(uint64_t n_nodes, const uint32_t *mirror, uint64_t n_edges,
                                const uint32_t *edge_from, const uint32_t *edge_to,
                                const uint64_t *edge_weight);
/* The clib.rs builder as three calls (matchtigs.h wraps exactly these). */
mtg_graph *mtg_graph_builder_new(uint64_t unitig_amount);
void mtg_graph_builder_merge(mtg_graph *g, uint64_t unitig_a, int strand_a, uint64_t unitig_b, int strand_b);
/* n links at once: row i = (unitig_a, strand_a, unitig_b, strand_b) as int64; the same unions in the same order as n merges. */
void mtg_graph_builder_merge_links(mtg_graph *g, uint64_t n_links, const int64_t *links);
void mtg_graph_builder_build(mtg_graph *g, const uint64_t *unitig_weights);
void mtg_graph_free(mtg_graph *g);
/* Removes every dummy edge again (undoes what compute_tigs appended), restoring the adjacency order of the
 * original graph exactly. The reference instead clones the graph before each algorithm (bin.rs:1069). */
void mtg_graph_reset(mtg_graph *g);
uint64_t mtg_graph_node_count(const mtg_graph *g);
uint64_t mtg_graph_edge_count(const mtg_graph *g); /* includes dummy edges added so far */
/* Copy out the current graph (any pointer may be NULL). forwards: 1/0. dummy_id 0 = original. */
void mtg_graph_export(const mtg_graph *g, uint32_t *mirror, uint32_t *edge_from, uint32_t *edge_to,
                      uint64_t *edge_weight, uint64_t *edge_dummy_id, uint64_t *edge_unitig,
                      uint8_t *edge_forwards);

/* The same for the edges [first_edge, first_edge + n_edges) only (large graphs: checks that stream over the edge arrays). */
void mtg_graph_export_range(const mtg_graph *g, uint64_t first_edge, uint64_t n_edges, uint32_t *edge_from, uint32_t *edge_to,
                            uint64_t *edge_weight, uint64_t *edge_dummy_id, uint64_t *edge_unitig, uint8_t *edge_forwards);
uint64_t mtg_graph_original_edge_count(const mtg_graph *g); /* edges before any dummy edge (2 x unitigs) */

/* ---- device stage ---------------------------------------------------------------------- */
/* Uploads the original edges to GPU `device_id` and builds the 64-byte family blocks for bound k-1 there.
 * Aborts if no GPU is present (there is no CPU path). Weights must be >= 1 for algorithm 5
 * (checked here; the reference's (distance, node) pop order needs it). */
mtg_device *mtg_device_create(const mtg_graph *g, uint64_t k, int device_id);
/* The same with options. MTG_DEVICE_NO_LOWER_BOUNDS: the goal-directed lower bounds (k <= 255, see mtg_sssp_count_visited) are NOT
 * computed with the graph -- they cost k - 1 passes over the nodes and a rewrite of the blocks, several times what they save ONE search;
 * the search then explores full balls (identical candidate lists). mtg_compute_tigs_cfg, whose device graph is searched once (the
 * reference's calling convention, clib.rs:291), builds it this way; a caller that holds an mtg_device and iterates keeps the default,
 * or adds the bounds later with mtg_device_build_lower_bounds (which repeats the classification if there was one).
 * mtg_device_lower_bounds_ms: GPU time (HIP events) of that precompute, 0 while the device graph has none.
 * MTG_DEVICE_RESERVE_WORK: for a caller that will STEP through the stages with this device graph (mtg_classify / mtg_sssp_candidates /
 * mtg_replay_claims_* / a finish on the same GPU), once or again and again: the device memory those stages take beside the graph
 * (about 60 bytes per node + 62 per edge at their peak) is taken from the driver now, in one piece, unless the library's arena holds it
 * already -- the first step then makes no driver allocation (it makes five otherwise, and single driver calls sporadically stall for
 * a second on shared hosts). Nothing is reserved if that would leave less than a sixth of the device to the process's other
 * allocators. Never changes a result. mtg_compute_tigs_cfg does not need it: its whole call is reserved when the graph is constructed. */
enum { MTG_DEVICE_DEFAULT = 0, MTG_DEVICE_NO_LOWER_BOUNDS = 1, MTG_DEVICE_RESERVE_WORK = 2 };
mtg_device *mtg_device_create_opts(const mtg_graph *g, uint64_t k, int device_id, int flags);
void mtg_device_build_lower_bounds(mtg_device *d, void *stream);
double mtg_device_lower_bounds_ms(const mtg_device *d);
void mtg_device_free(mtg_device *d);
/* Bytes of HBM held by the device graph. */
uint64_t mtg_device_graph_bytes(const mtg_device *d);

/* Node classification on the GPU. Returns the number of sources (out-nodes, ascending). */
uint64_t mtg_classify(mtg_device *d, void *stream);
/* Host copies of the classification (sizes: n_sources, n_nodes, n_nodes; any may be NULL). */
void mtg_classify_download(mtg_device *d, void *stream, uint32_t *out_nodes, int32_t *multiplicity,
                           uint8_t *is_in_node);
/* Device pointer to the ascending out-node list (uint32[n_sources]); valid until the next classify. */
const uint32_t *mtg_classify_d_out_nodes(const mtg_device *d);

/* Bounded many-to-many SSSP: for every source index i in [src_begin, src_end) writes its
 * candidate list L(s_i) = all in-nodes within k-1 of s_i (s_i excluded) as keys
 * (distance << 32 | node), ascending, into d_pool[d_cand_start[i-src_begin] ..+ d_cand_count[..]]
 * (d_cand_start of a source with d_cand_count 0 is left as it was: the start of an empty list means nothing).
 * Returns 0 on success; 1 if pool_capacity was too small (*pool_needed tells the size to retry
 * with; outputs are then invalid). Sources whose ball does not fit the fast kernel's LDS tables
 * are re-run by larger kernel levels internally, down to a dense level without any limit on the ball
 * (no legal input aborts: the reference's search has no size limit either, greedytigs/mod.rs:548-551).
 * k may exceed 65535 as long as every unitig weight stays below 65535 (weights are 16-bit in HBM).
 * Synchronises `stream` before returning. */
int mtg_sssp_candidates(mtg_device *d, void *stream, uint64_t src_begin, uint64_t src_end,
                        uint64_t *d_pool, uint64_t pool_capacity, uint64_t *d_cand_start,
                        uint32_t *d_cand_count, uint64_t *pool_needed);
/* Sum of the HIP-event durations (ms) of the SSSP level kernels of the last mtg_sssp_candidates call. */
double mtg_last_sssp_kernel_ms(const mtg_device *d);
/* Per level of that call: kernel duration (ms) and number of sources handed to the level. Level 0 is the
 * lane-per-source kernel (or the first cooperative level with preset 4); later levels re-run overflowed sources.
 * Returns the number of levels written (<= capacity). */
int mtg_last_sssp_levels(const mtg_device *d, double *ms_out, uint64_t *sources_out, int capacity);
/* Kernel instantiation that ran as level `level` of the last call ("" beyond the last level); valid until the next call. */
const char *mtg_last_sssp_level_name(const mtg_device *d, int level);
/* Runs the counting variant of the kernel (untimed instrumentation) over the same sources. */
void mtg_sssp_count(mtg_device *d, void *stream, uint64_t src_begin, uint64_t src_end, mtg_sssp_stats *stats);
/* Goal-directed pruning (k <= 255): with the device graph the engine computes lb(v) = distance from v to the nearest
 * initial in-node and lb+(v) = distance to the nearest one BEYOND v, and keeps weight + lb+(head) beside every edge weight and the
 * in-node flags of a node's children and grandchildren in its block. A search records an in-node it reaches at distance d <= k-1
 * from the block of its parent, and expands a node v -- reads its block, relaxes its out-edges -- only when d + lb+(v) <= k-1:
 * no in-node behind v can be within the bound otherwise, so the candidate lists are unchanged (the reference truncates its
 * searches as well, by target_amount, greedytigs/mod.rs:323-335); sources that cannot reach any in-node within the bound
 * are not searched at all. mtg_sssp_count keeps counting FULL balls (the unit of work of SURVEY 8d, equal to a full-ball
 * Dijkstra's counters); mtg_sssp_count_visited counts what the pruned search does: stats->sources = sources searched,
 * settled_nodes = distinct (source, node) pairs whose distance it determines, relaxed_edges = the out-edges of the pairs it
 * expands, emitted = the same candidates. Aborts when the device graph / plan does not prune (mtg_sssp_prunes() == 0). */
void mtg_sssp_count_visited(mtg_device *d, void *stream, uint64_t src_begin, uint64_t src_end, mtg_sssp_stats *stats);
int mtg_sssp_prunes(const mtg_device *d);
/* Sources the enumeration level of the last mtg_sssp_candidates call searched (0 when it does not prune). */
uint64_t mtg_last_sssp_searched_sources(const mtg_device *d);
/* Which SSSP level plan runs: 0 = default (table-free path enumeration per lane + sorting post-pass, then the cooperative
 * cascade for the sources it hands on; the level gathers its 64-byte node blocks per lane, or four lanes per block once the
 * blocks exceed 3 GB), 1 = cooperative cascade only (exact for any ball; the fallback plan and the one the counting kernels
 * use), 2 / 3 = plan 0 with the four-lanes-per-block / per-lane form of the gathers regardless of the graph's size (same
 * results; lets small graphs exercise both forms); 4 / 6 / 7 = plans 0 / 2 / 3 WITHOUT the goal-directed pruning (full balls, every
 * source searched; same results: A/B runs and tests); + 8 = the enumeration level on one workgroup (same results, slow: lets a test graph
 * of a few thousand sources take a wave through many chunks of sources). Returns the plan in force. */
int mtg_set_sssp_plan(mtg_device *d, int plan);

/* The claim loop (greedytigs/mod.rs:301-523, 1-thread order) on the GPU, over the candidate lists of ALL classified
 * sources (device arrays indexed by absolute source index, e.g. straight from mtg_sssp_candidates or an all-gather):
 * deterministic reservations by source index reproduce the sequential result exactly. Returns the number of pairs;
 * *pairs_out (HOST memory, malloc'd, free with mtg_free) holds them in the reference's push order. */
uint64_t mtg_replay_claims_device(mtg_device *d, void *stream, uint64_t n_sources, const uint64_t *d_cand_start,
                                  const uint32_t *d_cand_count, const uint64_t *d_pool, mtg_pair **pairs_out);
/* The same claim loop, but the pairs STAY in the HBM of d's GPU (no download): for a finish on the same GPU, which takes them from
 * there (mtg_finish_greedytigs_resident) -- mtg_compute_tigs_cfg works this way. Returns the number of pairs. They remain valid until
 * the next claim replay on d or mtg_device_free(d). */
uint64_t mtg_replay_claims_resident(mtg_device *d, void *stream, uint64_t n_sources, const uint64_t *d_cand_start,
                                    const uint32_t *d_cand_count, const uint64_t *d_pool);
/* Device pointer to those pairs (NULL when there are none) and their number. */
const mtg_pair *mtg_resident_pairs(const mtg_device *d, uint64_t *n_pairs_out);
/* A host copy of them (malloc'd, free with mtg_free), in the reference's push order. */
uint64_t mtg_download_resident_pairs(mtg_device *d, mtg_pair **pairs_out);
/* Geometry of the claim replay's cooperative launch, for measurements and tests (0 = the engine's choice for that parameter): number
 * of index-ordered admission windows (bits 0-15; bits 16-23: the sixteenth of them from which they grow, bits 24-31: by which factor
 * -- the engine's own choice is 36 windows, the second half twice as large), threads per workgroup (1024 or 256), workgroups, one admitting workgroup in `role_mod`, and
 * plain_barrier != 0 = every workgroup releases at the grid barrier (without the per-XCD stage that leans on gfx942 / gfx950
 * hardware). The pair list never depends on any of them. (The library reads no environment variable for this.) */
void mtg_set_replay_tuning(mtg_device *d, uint64_t windows, int block, int grid, int role_mod, int plain_barrier);
/* GPU time (HIP events, ms) of the last claim replay on d: [0] the rounds kernel (replay_rounds_kernel), [1] all of its GPU work
 * (state copy, dense list, rounds, pair-count scan, compaction). */
void mtg_last_replay_ms(const mtg_device *d, double out[2]);
/* Reservation rounds the last mtg_replay_claims_device needed. */
int mtg_last_replay_rounds(const mtg_device *d);
/* Source visits of those rounds (sum of the pending-list lengths): the unit of the replay's cost model. */
uint64_t mtg_last_replay_visits(const mtg_device *d);

/* ---- multi-GPU ------------------------------------------------------------- */
/* Two forms, by design:
 *  - INSIDE the library (this function, mtg_config.device_ids): ONE process drives n GPUs from n host threads, and the candidate
 *    lists travel to the first GPU as peer copies (hipMemcpyPeerAsync over xGMI: three copies per device, counts / starts / keys).
 *    The library does not link RCCL: a collective library adds nothing to a gather whose pieces already sit in one address space
 *    and whose replay order IS the device order, and it would make libmatchtigs.so depend on a communicator the reference's
 *    callers (clib.rs: one thread, no runtime) do not have.
 *  - ONE PROCESS PER GPU (matchtigs_amd/distributed.py, what bench.py runs under torch.distributed.run): the same exchange as
 *    grouped broadcasts at exact sizes over torch.distributed's "nccl" backend = RCCL over xGMI. This is the form north_star words
 *    ("RCCL all-gather of matched pairs"), and the only one in which ranks do not share an address space.
 * Both give the pair list of one GPU bit for bit (tests: gloo world 2 / 3, several resident copies on one GPU). Neither has run on
 * two distinct GPUs yet: the development pool hands out one GPU per job. */
/* SSSP + gather + claim replay over ALL classified sources of n_devices resident copies of the SAME graph (each created
 * with mtg_device_create on its GPU and classified): the ascending source list is cut into contiguous blocks of equal
 * estimated work (1 + out-degree of the source), device i searches block i from its own host thread, the candidate lists
 * are gathered on devices[0] with peer copies over xGMI (concatenation in device order is the replay order) and the claim
 * loop runs there. The pair list is identical for every n_devices. *pairs_out: host memory, free with mtg_free.
 * mtg_compute_tigs_cfg does exactly this for mtg_config.device_ids. */
uint64_t mtg_compute_pairs(mtg_device *const *devices, int n_devices, mtg_pair **pairs_out);
double mtg_last_gather_ms(void); /* wall-clock of the peer-copy gather of the last mtg_compute_pairs on this thread */
/* The block boundaries that split uses: cuts_out[0..parts], cuts_out[0] = 0, cuts_out[parts] = number of sources. */
void mtg_partition_sources(mtg_device *d, int parts, uint64_t *cuts_out);

/* ---- optimal matchtigs around the external matcher ---------------------------- */
/* matchtigs/mod.rs:150-940 minus the matcher itself. The reference runs one bounded Dijkstra per out-node with
 * target_amount = #in-nodes (:235-246) -- exactly the candidate lists of mtg_sssp_candidates -- and folds them into a
 * minimum-perfect-matching instance: collapsed matching nodes (GraphMatchingNodeMap, implementation/mod.rs:188-250), the
 * (min, max) -> (weight, out, target) edge map, two copies of that graph joined by weight-(k-1) edges, four extra nodes per
 * weakly connected component. The lists come from the GPU (cfg->device_ids[0]); the instance equals the reference's
 * threads == 1 result (with more threads the reference's node numbering depends on thread timing). */
typedef struct mtg_matching mtg_matching;
typedef struct {
    uint64_t transformed_node_count; /* matching nodes of one copy (:531) */
    uint64_t edge_count;             /* edges.len() (:535) */
    uint64_t wcc_amount;             /* WCCs that contain a matching node (:565) */
    uint64_t matching_node_count;    /* first number of the instance file (:598) */
    uint64_t matching_edge_count;    /* second number (:600) */
    uint64_t mirror_biedges, mirror_expanded_biedges; /* the two counts logged at :537-540 */
} mtg_matching_stats;
mtg_matching *mtg_matching_instance(const mtg_graph *g, const mtg_config *cfg);
/* The host stage alone, over candidate lists the caller holds (layout of mtg_replay_claims; multiplicity as downloaded by
 * mtg_classify_download: negative for out-nodes). */
mtg_matching *mtg_matching_instance_from_lists(const mtg_graph *g, uint64_t k, uint64_t n_sources, const uint32_t *out_nodes,
                                               const int32_t *multiplicity, const uint64_t *cand_start,
                                               const uint32_t *cand_count, const uint64_t *pool);
void mtg_matching_get_stats(const mtg_matching *m, mtg_matching_stats *out);
/* Writes the instance text (:591-719) to `path`; returns the bytes written. */
uint64_t mtg_matching_write(const mtg_matching *m, const char *path);
/* Reads a matcher solution (:746-812): the matched pairs (original out-node, in-node, weight) in file order, ready for
 * mtg_finish_matchtigs_cfg. *pairs_out: malloc'd, free with mtg_free. Aborts on an edge that is not in the instance (:794). */
uint64_t mtg_matching_read_solution(const mtg_matching *m, const char *solution_path, mtg_pair **pairs_out);
void mtg_matching_free(mtg_matching *m);
/* Inserts the matched edges, Eulerises, walks and cuts (:797-935): mtg_finish_greedytigs_cfg plus the reference's assertion
 * that every bicycle with a dummy edge holds a breaking edge (:883). */
mtg_walks *mtg_finish_matchtigs_cfg(mtg_graph *g, const mtg_pair *pairs, uint64_t n_pairs, const mtg_config *cfg);
/* The whole algorithm (tig algorithm 4 of mtg_compute_tigs_cfg): instance -> cfg->matcher_path as a child process ->
 * solution -> matchtigs. */
mtg_walks *mtg_compute_matchtigs_cfg(mtg_graph *g, const mtg_config *cfg);

/* ---- host stages ----------------------------------------------------------------------- */
/* Replays the reference's claim loop over the candidate lists in ascending source order.
 * cand_start/cand_count index `pool`. multiplicity / is_in_node are the classification
 * (copied, not modified). Returns the number of pairs; *pairs_out is malloc'd (mtg_free). */
uint64_t mtg_replay_claims(const mtg_graph *g, uint64_t n_sources, const uint32_t *out_nodes,
                           const int32_t *multiplicity, const uint8_t *is_in_node,
                           const uint64_t *cand_start, const uint32_t *cand_count,
                           const uint64_t *pool, mtg_pair **pairs_out);
void mtg_free(void *p);

/* Dummy insertion + Eulerisation + Euler decomposition + cut. Mutates g like the reference. */
mtg_walks *mtg_finish_greedytigs(mtg_graph *g, const mtg_pair *pairs, uint64_t n_pairs, uint64_t k);
mtg_walks *mtg_compute_eulertigs(mtg_graph *g, uint64_t k);
/* Sub-stages, exported for parity tests. */
uint64_t mtg_insert_pair_edges(mtg_graph *g, const mtg_pair *pairs, uint64_t n_pairs); /* returns last dummy id */
uint64_t mtg_make_eulerian(mtg_graph *g, uint64_t dummy_edge_id, uint64_t k);          /* returns last dummy id */
mtg_walks *mtg_euler_cycles(const mtg_graph *g);
/* The same walk over the record formats the device finish feeds it, with the records built on the host from the
 * graph's adjacency lists: 1 = 32-byte records (euler_lean.cpp), 2 = 256-byte records seeded from 32-byte ones. Same sequences as
 * mtg_euler_cycles (format 0); exported for the CPU test suite and the sanitizer builds. */
mtg_walks *mtg_euler_cycles_records(const mtg_graph *g, int record_format);
mtg_walks *mtg_cut_cycles(const mtg_graph *g, const mtg_walks *cycles, uint64_t k);
/* the Euler bicycles computed on the GPU by a parallel algorithm (trail pairing, union-find merge,
 * list ranking). Same guarantees as the reference's decomposition (greedytigs/mod.rs:722: one closed biwalk per
 * connected component, every biedge exactly once in one orientation) but NOT the reference's walk order, so tig
 * boundaries differ while #tigs and cumulative length stay the same (SURVEY 8a invariance note). Opt-in:
 * mode 0 (default) = host walk in the reference's order, mode 1 = this. Aborts without a GPU. */
mtg_walks *mtg_euler_cycles_device(const mtg_graph *g, int device_id);
double mtg_last_euler_kernel_ms(void); /* of the last device decomposition on this thread */
/* The decomposition's segment walks recognise a splitter by a mark in bit 31 of its predecessor's successor word while dart ids
 * leave that bit free (fewer than 2^31 darts), else by a bitmap lookup per step. Bit 0 of `flags` forces the bitmap form, bit 1 ranks
 * the reduced list by pointer jumping over ALL splitters instead of two levels, bit 2 writes the closed walks by a second walk through
 * the successor array instead of from the sequence the measuring walk recorded, bit 3 shrinks the per-wave chunk tables of that
 * record to one entry, so that large graphs take the fallback to the second walk (process-wide; tests hold the forms to the same walks). */
void mtg_set_euler_device_tuning(int flags);
/* The whole finish on the GPU for a graph that holds only its original edges (finish_device.hip): matched-pair darts, the
 * Euleriser in the reference's sequence (implementation/mod.rs:392-649), Euler bicycles per cfg->euler_mode (device
 * decomposition, or the reference-order host walk over GPU-built records), rotate + cut (greedytigs/mod.rs:726-789). Appends the
 * dummy edges to g like the host stages do (same ids, weights and dummy ids). n_pairs == 0 is the Eulertig finish. */
mtg_walks *mtg_finish_device(mtg_graph *g, const mtg_pair *pairs, uint64_t n_pairs, const mtg_config *cfg);
/* mtg_finish_greedytigs_cfg with the matched pairs the last claim replay on `d` left in HBM (mtg_replay_claims_resident): when the
 * finish runs on d's GPU (cfg->device_ids[0], finish_stage AUTO / DEVICE, a graph without dummy edges) nothing is uploaded and
 * only the dummy weights come down, beside the GPU stages; otherwise the pairs take the way through the host. Same tigs either way. */
mtg_walks *mtg_finish_greedytigs_resident(mtg_graph *g, mtg_device *d, const mtg_config *cfg);
/* Device memory the library keeps BETWEEN calls, and how to get it back:
 *  - the finishing stages keep the work arrays of the last call on a GPU for the next one (a caller that finishes graph after graph
 *    pays no allocation); a call frees what it did not touch itself, so at most one call's arrays are held, and calls that worked
 *    on more than a third of the device's memory keep nothing. mtg_device_memory_held tells how much that is right now, mtg_release_device_memory gives
 *    all of it back to the driver (e.g. before another allocator of the process needs the HBM);
 *  - a graph keeps the device copy of its original edges, its mirror array and the buckets of its original darts on the GPU of
 *    its first device stage (<= 8 B per edge + 8 B per node) until mtg_graph_free / mtg_graph_release_device_cache.
 * Neither changes a result; the next call simply allocates / uploads again. */
void mtg_release_device_memory(int device_id);
uint64_t mtg_device_memory_held(int device_id);
/* The arena of that GPU in numbers: out[0] bytes in chunks taken from the driver, [1] bytes of live arrays, [2] their peak since the last
 * reset, [3] driver allocations made so far. reset_peak != 0: the peak restarts at what is live now (measurements: what a stage needs). */
void mtg_device_arena_stats(int device_id, uint64_t out[4], int reset_peak);
void mtg_graph_release_device_cache(mtg_graph *g);
/* The GPU whose memory a graph's construction reserves ahead of the call that will follow (default 0): building a graph of more
 * than a few million edges (mtg_graph_from_edges, matchtigs_initialise_graph, mtg_synth_g_csr on its own device) starts a helper
 * thread that brings up the HIP runtime, loads the kernels and takes ONE chunk of device memory sized for the whole call from
 * (nodes, edges) -- every device array of the call is then a range of it (hip_util.hpp: DeviceArena), so no stage waits for the
 * driver. A process that runs one rank per GPU names its GPU here before it builds graphs. Never changes a result; without a GPU
 * nothing happens. */
void mtg_set_default_device(int device_id);
/* on = 0: host-only graph constructors (mtg_graph_from_edges, matchtigs_initialise_graph) start no helper thread and reserve nothing
 * on any GPU -- for callers that want them free of GPU side effects; the first computing call then reserves for itself. Default 1.
 * Either way a reservation is provisional: a call that computes on other GPUs than the one it was made on gives it back when it
 * ends, and the helper threads are joined (each new one joins those that are through, the library's teardown joins the rest). */
void mtg_set_reserve_ahead(int on);
/* Tuning of the finishing stages for measurements and tests (process-wide, read at the start of a call; the library reads no
 * environment variable for any of it, and none changes a result). records: walk-record format of the reference-order mode, 0 = the
 * engine's choice by size and host memory, 1 = 32-byte, 2 = 128-byte, 3 = 256-byte records. flags: bit 0 = the walk
 * waits until all of its records have arrived (instead of starting on the 32-byte ones), bit 1 = never page-lock the record arena,
 * bit 2 = keep nothing of a graph on the device between calls (edges, mirror, buckets), bit 3 = a trivial kernel every 2 ms while the
 * host walks in the reference's order (measurement: what the GPU's idle state costs the first kernels of the next step), bit 4 = the device
 * Euler mode builds the closed walks of every component even where the tigs can be cut straight from the pairing (cut_first_device.hip; tests and
 * A/B measurements -- the tigs of that mode then come in another order, which the mode leaves unspecified, with the same count and cumulative
 * length). record_delay_us: slows the arrival of the
 * records by that much per slice (tests: small graphs then take the 32-byte path for most of their steps). */
void mtg_set_finish_tuning(int records, int flags, int64_t record_delay_us);
/* Seconds of the last mtg_finish_device on this thread: [0] upload + insertion + Euleriser, [1] dummy edges into the host graph,
 * [2] Euler bicycles, [3] rotate + cut + tig download; [4] kernel ms of the device decomposition; [5] breaking biedges added. */
void mtg_last_finish_device_times(double out[6]);
/* GPU time (HIP events on the finish stream, ms) of the stages of the last mtg_finish_device on this thread, for the per-stage
 * rooflines of bench.py: [0] matched-pair darts + Euleriser kernels, [1] buckets + walk records (reference-order mode),
 * [2] Euler decomposition (device mode), [3] rotate + cut kernels (without the tig download); [4] darts after the finish,
 * [5] Euleriser units (missing in-edges). */
void mtg_last_finish_device_stage_ms(double out[6]);
/* The two finishing paths with an explicit configuration (euler_mode, finish_stage, device_ids[0]). */
mtg_walks *mtg_finish_greedytigs_cfg(mtg_graph *g, const mtg_pair *pairs, uint64_t n_pairs, const mtg_config *cfg);
mtg_walks *mtg_compute_eulertigs_cfg(mtg_graph *g, const mtg_config *cfg);

/* A walk set. The tigs of a finish on the GPU (finish_stage auto / device) stay in that GPU's memory until a call needs them on the
 * host: the two counts below never copy; mtg_walks_export, mtg_walks_data, mtg_flatten_clib, the duplication bit vectors and the host
 * writers bring them over once (0.37 GB at the human-like bench size, through the pinned transfer ring) and release the device
 * arrays; mtg_write_tigs_text_file_device spells them in place when asked for the same GPU; mtg_walks_free of an unread handle copies
 * nothing. One thread per handle. */
uint64_t mtg_walks_count(const mtg_walks *w);
uint64_t mtg_walks_total_edges(const mtg_walks *w);
/* limits[i] = exclusive end of walk i in edges[] (edge ids into the mutated graph). */
void mtg_walks_export(const mtg_walks *w, uint64_t *limits, uint32_t *edges);
/* The walks' own arrays (no copy): valid until mtg_walks_free. */
void mtg_walks_data(const mtg_walks *w, const uint64_t **limits, const uint32_t **edges);
void mtg_walks_free(mtg_walks *w);
/* Walks from caller arrays (copied), e.g. externally computed Euler cycles for mtg_cut_cycles. */
mtg_walks *mtg_walks_from_arrays(uint64_t n_walks, const uint64_t *limits, const uint32_t *edges);

/* clib.rs:393-407 flattening into caller arrays sized as clib.rs:332-348. Returns #tigs. */
uint64_t mtg_flatten_clib(const mtg_graph *g, const mtg_walks *tigs, int64_t *tigs_edge_out,
                          uint64_t *tigs_insert_out, uint64_t *tigs_out_limits);

/* Tig spelling (replaces write_walks_fasta, bin.rs:466-606): walks (edge ids into the mutated graph,
 * limits[i] = exclusive end of walk i) -> FASTA text. unitig_seqs = concatenated ASCII sequences, unitig u occupies
 * [seq_offsets[u], seq_offsets[u+1]). Header ">{i+1}"; overlaps k-1 after a unitig edge, k-1-weight after a dummy
 * edge; backwards edges are reverse-complemented. Returns the byte count; *fasta_out is malloc'd (mtg_free).
 * Aborts with a message where the reference panics: an empty walk, a walk whose first edge is a dummy, a dummy edge heavier than
 * k-1 in front of a unitig edge, an overlap longer than the unitig (the same checks, before any GPU call, in the _gfa and _device
 * forms below). */
uint64_t mtg_write_walks_fasta(const mtg_graph *g, uint64_t n_walks, const uint64_t *limits, const uint32_t *edges,
                               uint64_t k, const char *unitig_seqs, const uint64_t *seq_offsets, char **fasta_out);

/* BCALM2 / GGCAT unitig FASTA input (the `--bcalm-in X -k K` route, bin.rs:902-912): every
 * `L:<strand>:<id>:<strand>` annotation becomes one merge of unitig ends exactly as matchtigs_merge_nodes does
 * (clib.rs:135-170), weights are len + 1 - k (bin.rs:369). `.gz` files are inflated. Returns the built graph and the
 * sequence store (free with mtg_unitigs_free). Aborts on malformed input, non-ACGT characters, sequences shorter than k. */
typedef struct mtg_unitigs mtg_unitigs;
mtg_graph *mtg_read_bcalm2(const char *path, uint64_t k, mtg_unitigs **unitigs_out);
/* Plain unitig FASTA input (the `--fa-in X -k K` route, bin.rs:71-75, 891-901): no topology in the file -- every pair of unitig
 * ends that share a (k-1)-mer, in either orientation, is joined on GPU `device_id` (there is no CPU path). Nodes are oriented
 * (k-1)-mers numbered in first-occurrence order of their class {x, rc(x)} (first k-1 bases of record u = occurrence
 * 2u, last k-1 = 2u + 1); edges 2u / 2u+1 as above, weight len + 1 - k. Headers may hold any text (`L:` annotations are ignored),
 * sequences may span lines and be lower case, `.gz` files are inflated. Aborts on non-ACGT characters, records shorter than k,
 * k < 2 and graphs past the 32-bit ids. */
mtg_graph *mtg_read_fasta(const char *path, uint64_t k, int device_id, mtg_unitigs **unitigs_out);
/* The same join over records held in memory: record u is data[offsets[u], offsets[u + 1]), offsets[0] = 0 (n + 1 offsets, the
 * layout of mtg_unitigs_data / _offsets). */
mtg_graph *mtg_graph_from_sequences(const char *data, const uint64_t *offsets, uint64_t n, uint64_t k, int device_id);
/* Of the last mtg_read_fasta / mtg_graph_from_sequences on this thread: {parse ms (0 for the in-memory entry), upload ms, join
 * kernels ms (HIP events), download ms, graph build ms, bytes the join kernels must move at the least}. */
void mtg_last_fasta_in_times(double out[6]);
/* Any FASTA file (optionally `.gz`; headers with any text, sequences on one or more lines, either case) as a sequence store: no graph
 * and no length rule -- a record shorter than k is legal in a file another tool wrote. Aborts on non-ACGT characters. */
void mtg_read_sequences(const char *path, mtg_unitigs **store_out);
/* Do two sequence sets hold the same k-mers? (kmer_compare_device.hip). A set is concatenated ASCII plus n + 1 offsets
 * (offsets[0] = 0; the layout of mtg_unitigs_data / _offsets). Its k-mers are the windows of length k inside one record, compared by
 * their canonical form (the lexicographically smaller of x and rc(x), A < C < G < T; lower case equals upper case). Records shorter
 * than k contribute nothing; k >= 1, even k included; a character outside ACGT aborts. Exact (no probabilistic structure) and a
 * function of the inputs alone. Computed on GPU `device_id`: there is no CPU path. Limit: fewer than 2^40 - 1 bases in A and B
 * together. The sets are equal iff only_in_a == only_in_b == 0; B repeats occurrences_b - distinct_b k-mers. */
typedef struct mtg_kmer_comparison {
    uint64_t records_a, records_b;         /* as given */
    uint64_t characters_a, characters_b;   /* as given */
    uint64_t occurrences_a, occurrences_b; /* windows: sum over the records of max(0, len - k + 1) */
    uint64_t distinct_a, distinct_b;       /* distinct canonical k-mers */
    uint64_t common, only_in_a, only_in_b; /* sizes of A and B, A without B, B without A: distinct_a = common + only_in_a, likewise for b */
    /* the occurrence in A with the smallest (record, position) whose k-mer is not in B; UINT64_MAX when there is none */
    uint64_t first_only_in_a_record, first_only_in_a_pos;
    uint64_t first_only_in_b_record, first_only_in_b_pos; /* the same for B */
} mtg_kmer_comparison;
void mtg_compare_kmer_sets(const char *seq_a, const uint64_t *off_a, uint64_t n_a, const char *seq_b, const uint64_t *off_b,
                           uint64_t n_b, uint64_t k, int device_id, mtg_kmer_comparison *out);
/* The same over two stores as mtg_read_bcalm2 / mtg_read_fasta / mtg_read_sequences hand them out. */
void mtg_compare_kmer_sets_stores(const mtg_unitigs *store_a, const mtg_unitigs *store_b, uint64_t k, int device_id,
                                  mtg_kmer_comparison *out);
/* Of the last comparison on this thread, in ms: {upload (host clock), pack, insert A (with the table's fill), insert B, count (with
 * the witness passes, when there is a difference) -- HIP events around the kernels --, the whole call (host clock)}. */
void mtg_last_kmer_compare_times(double out[6]);
/* mtg_read_sequences where a run of characters outside ACGT (the `N` of real assemblies) ends a piece instead of aborting: every
 * maximal ACGT stretch of a record becomes a record of the store, in file order; empty pieces are dropped. *pieces_cut (may be NULL)
 * = the runs met. */
void mtg_read_sequences_split(const char *path, mtg_unitigs **store_out, uint64_t *pieces_cut);
/* The maximal unitigs of the k-mer set of arbitrary sequences, compacted on GPU `device_id` (compact_device.hip; there
 * is no CPU path). Input: concatenated ASCII plus n + 1 offsets (offsets[0] = 0), either case; a window is a start position whose k
 * bases lie inside one record, records shorter than k contribute nothing, a character outside ACGT aborts. S = the canonical k-mers
 * of all windows. creator(x) = the smallest window start (in the concatenation) whose k-mer is x or rc(x); reading(x) = the string
 * there. The graph is the one mtg_graph_from_sequences builds from the readings (oriented (k-1)-mers as nodes, each k-mer the edge
 * prefix -> suffix and its mirror). A node is passable iff it is not its own mirror and has in-degree 1 and out-degree 1 over all
 * directed edges; a unitig is a maximal walk whose inner nodes are passable, closed when the node between its last and first edge is
 * passable too. Its leader is its k-mer with the smallest creator; of the walk and its mirror the one on which the leader appears as
 * reading(leader) is emitted, a closed walk starting at its leader and spelled linearly; unitigs come in increasing order of their
 * leaders' creators, upper case, edges + k - 1 characters each. The result is a function of the input alone. *out is an ordinary
 * store (mtg_unitigs_free) that mtg_graph_from_sequences, the writers and mtg_compare_kmer_sets_stores accept. 2 <= k < 2^31, fewer
 * than 2^40 - 1 bases, fewer than 2^31 - 1 distinct k-mers. */
typedef struct mtg_compaction {
    uint64_t records, characters; /* as given */
    uint64_t windows;             /* sum over the records of max(0, len - k + 1) */
    uint64_t distinct_kmers;      /* |S| = unitig_characters - (k - 1) * unitigs */
    uint64_t unitigs, unitig_characters;
    uint64_t closed_walks;        /* unitigs whose walk is closed */
    uint64_t longest_unitig_kmers;
} mtg_compaction;
void mtg_compact_unitigs(const char *data, const uint64_t *offsets, uint64_t n, uint64_t k, int device_id, mtg_unitigs **out,
                         mtg_compaction *stats);
/* The same over a store as mtg_read_sequences / mtg_read_sequences_split hand it out. */
void mtg_compact_unitigs_store(const mtg_unitigs *in, uint64_t k, int device_id, mtg_unitigs **out, mtg_compaction *stats);
/* Of the last compaction on this thread, counted or not: {upload ms (host clock); pack, insert, ids, nodes (with succ), rank (pointer jumping), emit
 * ms -- HIP events around the kernel phases --; download ms and the whole call (host clock); pointer-jumping rounds; bytes the
 * kernels must move at the least; peak of live device-arena bytes}. */
void mtg_last_compact_times(double out[12]);
/* The compaction with an abundance threshold. abundance(x), for a canonical k-mer x, = the number of windows whose
 * k-mer is x or rc(x): repeats inside a record count, both strands count, a window whose k-mer is its own reverse complement counts
 * once. S_m = { x : abundance(x) >= min_abundance }. creator(x) and reading(x) stay what mtg_compact_unitigs says, taken over ALL
 * windows of the input; the rest of its contract (graph, passable nodes, unitigs, leaders, order, spelling) applies to S_m with those
 * creators -- the removed k-mers take their edges with them. With min_abundance = 1 the store and `stats` are byte for byte those of
 * mtg_compact_unitigs. stats->distinct_kmers = |S_m|; stats->windows stays the input's windows. *sums holds, per unitig in the
 * store's record order, the sum of abundance over its k-mers; their total is kept_occurrences. Exact integers, a function of the
 * input and min_abundance alone. An empty S_m gives an empty store. min_abundance >= 1; fewer than 2^32 windows (the counters are
 * 32-bit and must not wrap); both abort with a message otherwise. */
typedef struct mtg_abundance {
    uint64_t distinct_all;     /* |S_1| */
    uint64_t distinct_kept;    /* |S_m| */
    uint64_t max_abundance;
    uint64_t kept_occurrences; /* sum of abundance over S_m */
    uint64_t spectrum[256];    /* over S_1: [c] = distinct k-mers with abundance c (1 <= c <= 254), [255] = with abundance >= 255, [0] = 0 */
} mtg_abundance;
typedef struct mtg_abundance_sums mtg_abundance_sums;
void mtg_compact_unitigs_counted(const char *data, const uint64_t *offsets, uint64_t n, uint64_t k, uint64_t min_abundance, int device_id,
                                 mtg_unitigs **out, mtg_compaction *stats, mtg_abundance *abundance,
                                 mtg_abundance_sums **sums); /* mtg_abundance_sums_free */
void mtg_compact_unitigs_counted_store(const mtg_unitigs *in, uint64_t k, uint64_t min_abundance, int device_id, mtg_unitigs **out,
                                       mtg_compaction *stats, mtg_abundance *abundance, mtg_abundance_sums **sums);
uint64_t mtg_abundance_sums_count(const mtg_abundance_sums *sums);        /* the store's unitigs */
const uint64_t *mtg_abundance_sums_array(const mtg_abundance_sums *sums); /* count entries; valid until mtg_abundance_sums_free */
void mtg_abundance_sums_free(mtg_abundance_sums *sums);
/* mtg_compact_unitigs_counted, output for output, plus the abundance of every kept k-mer: *kmer_counts holds one
 * uint32 per k-mer of S_m IN WINDOW ORDER OF THE OUTPUT STORE -- entry (sum over the unitigs v < u of len(v) - k + 1) + j is the
 * abundance of the k-mer at offset j of unitig u; count = distinct_kept, the entries of unitig u add up to sums[u]. It is the weights
 * array mtg_kmer_index_build_weighted_store takes for *out. An empty S_m gives a handle with zero entries. */
typedef struct mtg_kmer_counts mtg_kmer_counts;
void mtg_compact_unitigs_counted_kmers(const char *data, const uint64_t *offsets, uint64_t n, uint64_t k, uint64_t min_abundance, int device_id,
                                       mtg_unitigs **out, mtg_compaction *stats, mtg_abundance *abundance, mtg_abundance_sums **sums,
                                       mtg_kmer_counts **kmer_counts); /* mtg_kmer_counts_free */
void mtg_compact_unitigs_counted_kmers_store(const mtg_unitigs *in, uint64_t k, uint64_t min_abundance, int device_id, mtg_unitigs **out,
                                             mtg_compaction *stats, mtg_abundance *abundance, mtg_abundance_sums **sums,
                                             mtg_kmer_counts **kmer_counts);
uint64_t mtg_kmer_counts_count(const mtg_kmer_counts *counts);        /* the store's k-mers */
const uint32_t *mtg_kmer_counts_array(const mtg_kmer_counts *counts); /* count entries; valid until mtg_kmer_counts_free */
void mtg_kmer_counts_free(mtg_kmer_counts *counts);
/* A k-mer set kept on GPU `device_id` and asked which k-mers of other sequences it holds (kmer_query_device.hip; there
 * is no CPU path). The indexed set is a set in mtg_compare_kmer_sets' sense: the canonical k-mers of the windows of length k inside
 * one record; records shorter than k contribute nothing, a character outside ACGT aborts, k >= 1. The index holds device memory
 * (info.device_bytes) until mtg_kmer_index_free; mtg_release_device_memory leaves it intact. Limits: fewer than 2^40 - 1 bases in
 * the index and in one query call, k < 2^32. */
typedef struct mtg_kmer_index mtg_kmer_index;
typedef struct mtg_kmer_index_info {
    uint64_t k, records, characters; /* as given */
    uint64_t occurrences;            /* windows: sum over the records of max(0, len - k + 1) */
    uint64_t distinct;               /* distinct canonical k-mers */
    uint64_t slots, device_bytes;    /* of the table; what the index keeps on the device */
} mtg_kmer_index_info;
mtg_kmer_index *mtg_kmer_index_build(const char *seq, const uint64_t *off, uint64_t n, uint64_t k, int device_id);
/* The same over a store as mtg_read_bcalm2 / mtg_read_fasta / mtg_read_sequences / mtg_compact_unitigs hand it out. */
mtg_kmer_index *mtg_kmer_index_build_store(const mtg_unitigs *store, uint64_t k, int device_id);
void mtg_kmer_index_get_info(const mtg_kmer_index *ix, mtg_kmer_index_info *out);
/* The query: n records of ARBITRARY bytes (concatenated plus n + 1 offsets, off[0] = 0). For record r of length L: kmers[r] =
 * max(0, L - k + 1); a window is valid iff all k of its characters are in ACGTacgt; valid[r] = the valid windows, found[r] = the
 * valid windows whose canonical form is in the index. present_bits / valid_bits (each may be NULL; (off[n] + 63) / 64 words): over
 * the global base positions of the query, bit p & 63 of word p >> 6 of valid_bits is set iff a valid window starts at p, of
 * present_bits iff that window is in the index; every other bit is 0. Exact integers, a function of the inputs alone; the index is
 * not changed. An empty index finds nothing; an empty query returns at once. */
void mtg_kmer_index_query(const mtg_kmer_index *ix, const char *seq, const uint64_t *off, uint64_t n,
                          uint64_t *kmers, uint64_t *valid, uint64_t *found, /* [n] each */
                          uint64_t *present_bits, uint64_t *valid_bits);     /* nullable */
void mtg_kmer_index_free(mtg_kmer_index *ix);
/* Of the last index build and the last query on this thread, in ms: {build: upload (host clock), pack, insert (with the table's fill
 * and the count); query: upload (host clock), pack, probe} -- HIP events around the kernels. */
void mtg_last_kmer_query_times(double out[6]);
/* The same question asked of a SPARSE index (tig_index_device.hip; there is no CPU path): instead of a table slot per
 * window it keeps the 2-bit packed bases, the record offsets and one 8-byte word per minimizer anchor -- about 2 / (k - m + 2) of the
 * windows --, so its size follows the cumulative length of the indexed sequences: tigs index smaller than unitigs. m is the
 * minimizer length, 1 <= m <= min(k, 31); m = 0 means min(19, ceil(2 k / 3)). A directory bucket with more than bucket_limit anchors
 * (low-complexity minimizers) is heavy: its windows go into a class table of 16 B per window instead; bucket_limit = 0 means 64, and
 * 65536 is the most. Membership is decided by a compare of packed bases: exact, like the table index. The index holds device
 * memory (info.device_bytes) until mtg_tig_index_free; mtg_release_device_memory leaves it intact. Limits: those of mtg_kmer_index. */
typedef struct mtg_tig_index mtg_tig_index;
typedef struct mtg_tig_index_info {
    uint64_t k, m, records, characters, occurrences;    /* as mtg_kmer_index_info; m as used */
    uint64_t anchors, buckets, bucket_limit;            /* anchors kept, directory buckets (a power of two), the limit as used */
    uint64_t heavy_buckets, heavy_windows, table_slots; /* the skew path: buckets over the limit, windows in the table, its slots */
    uint64_t device_bytes;                              /* everything the index keeps on the device */
} mtg_tig_index_info;
mtg_tig_index *mtg_tig_index_build(const char *seq, const uint64_t *off, uint64_t n, uint64_t k, uint64_t m, uint64_t bucket_limit,
                                   int device_id);
mtg_tig_index *mtg_tig_index_build_store(const mtg_unitigs *store, uint64_t k, uint64_t m, uint64_t bucket_limit, int device_id);
void mtg_tig_index_get_info(const mtg_tig_index *ix, mtg_tig_index_info *out);
/* mtg_kmer_index_query's contract, word for word: the same outputs for the same indexed set and query. */
void mtg_tig_index_query(const mtg_tig_index *ix, const char *seq, const uint64_t *off, uint64_t n,
                         uint64_t *kmers, uint64_t *valid, uint64_t *found, /* [n] each */
                         uint64_t *present_bits, uint64_t *valid_bits);     /* nullable */
void mtg_tig_index_free(mtg_tig_index *ix);
/* Of the last tig index build and the last query of one on this thread, in ms: {build: upload (host clock), pack, anchors (mark,
 * count, compact), directory (histogram, scan, scatter, sort), heavy table (count, insert); query: upload (host clock), pack, probe}
 * -- HIP events around the kernels. */
void mtg_last_tig_index_times(double out[8]);
/* WHERE the k-mers of a query are in the indexed sequences. A LOCATING index is built by the two functions below;
 * beside the table it keeps the smallest position of every class, the packed bases (for every k) and the record offsets, all counted
 * in info.device_bytes. mtg_kmer_index_query answers on it exactly as on a plain index. */
mtg_kmer_index *mtg_kmer_index_build_locating(const char *seq, const uint64_t *off, uint64_t n, uint64_t k, int device_id);
mtg_kmer_index *mtg_kmer_index_build_locating_store(const mtg_unitigs *store, uint64_t k, int device_id);
int mtg_kmer_index_is_locating(const mtg_kmer_index *ix);
/* The query of mtg_kmer_index_query (kmers / valid / found as there) plus the maximal collinear runs of its found windows. For a
 * found window w: loc(w) = the smallest global start position, in the index's concatenated bases, of a window of w's class;
 * strand(w) = + iff the upper-cased query window equals the index window there base by base, else - (a palindrome is +). Window p
 * continues window p - 1 iff both start in the same query record, both are found, have the same strand, loc(p) = loc(p - 1) + 1
 * (+) or loc(p - 1) - 1 (-), and both locations lie in the same index record. A run starts at every found window that does not
 * continue its predecessor; runs come in ascending query position. Per run: q_record, q_start (offset of its first window in that
 * record), kmers (windows), strand (0 = +, 1 = -), t_record (0-based index record) and t_start (offset in it of the leftmost index
 * base the run covers): query bases [q_start, q_start + kmers + k - 1) equal index bases [t_start, t_start + kmers + k - 1) of
 * t_record, case-insensitively, for - as the reverse complement. A k-mer that occurs more than once is reported at its smallest
 * position only, so repeats break runs. Exact integers, a function of the inputs alone. Dies if the index is not locating. */
typedef struct mtg_kmer_runs mtg_kmer_runs;
void mtg_kmer_index_locate(const mtg_kmer_index *ix, const char *seq, const uint64_t *off, uint64_t n,
                           uint64_t *kmers, uint64_t *valid, uint64_t *found, /* [n] each */
                           mtg_kmer_runs **out);                              /* mtg_kmer_runs_free */
uint64_t mtg_kmer_runs_count(const mtg_kmer_runs *runs);
/* count entries each; valid until mtg_kmer_runs_free */
void mtg_kmer_runs_arrays(const mtg_kmer_runs *runs, const uint64_t **q_record, const uint64_t **q_start, const uint64_t **kmers,
                          const uint8_t **strand, const uint64_t **t_record, const uint64_t **t_start);
void mtg_kmer_runs_free(mtg_kmer_runs *runs);
/* Of the last mtg_kmer_index_locate on this thread, in ms: {upload (host clock), pack, probe (with the fill of the hit array), runs
 * (flag, scan, emit)} -- HIP events around the kernels. */
void mtg_last_kmer_locate_times(double out[4]);
/* The same answer from the SPARSE index. A LOCATING tig index is built by the two functions below; beside what a
 * plain one keeps it holds the smallest position of every class of its heavy buckets, 8 B per table slot, counted in
 * info.device_bytes -- nothing more where no bucket is heavy. mtg_tig_index_query answers on it exactly as on a plain index.
 * mtg_tig_index_locate is mtg_kmer_index_locate's contract, word for word, "the index" being the sequences the tig index was built
 * from: for the same sequences, query and k the counts and the runs are field for field those of a locating mtg_kmer_index, for every
 * m and bucket_limit. It dies if the index is not locating (build it with mtg_tig_index_build_locating). */
mtg_tig_index *mtg_tig_index_build_locating(const char *seq, const uint64_t *off, uint64_t n, uint64_t k, uint64_t m,
                                            uint64_t bucket_limit, int device_id);
mtg_tig_index *mtg_tig_index_build_locating_store(const mtg_unitigs *store, uint64_t k, uint64_t m, uint64_t bucket_limit, int device_id);
int mtg_tig_index_is_locating(const mtg_tig_index *ix);
void mtg_tig_index_locate(const mtg_tig_index *ix, const char *seq, const uint64_t *off, uint64_t n,
                          uint64_t *kmers, uint64_t *valid, uint64_t *found, /* [n] each */
                          mtg_kmer_runs **out);                              /* mtg_kmer_runs_count / _arrays / _free */
/* Of the last mtg_tig_index_locate on this thread, in ms: {upload (host clock), pack, probe (with the fill of the hit array), runs
 * (flag, scan, emit)} -- HIP events around the kernels. */
void mtg_last_tig_locate_times(double out[4]);
/* WHICH PATH through the indexed records a query takes: the runs of mtg_kmer_index_locate joined across record ends
 * into walks. Let W(u) = len(u) - k + 1 be the windows of index record u. A run (q_record, q_start, n = kmers, strand, u = t_record,
 * t = t_start) ENTERS AT THE HEAD of u iff t == 0 (+) or t + n == W(u) (-), and LEAVES AT THE TAIL iff t + n == W(u) (+) or t == 0
 * (-). Run r + 1 CONTINUES run r iff both have the same q_record, q_start[r + 1] == q_start[r] + n[r], r leaves at the tail and
 * r + 1 enters at the head: the query being contiguous there, the last k - 1 bases of step r, as oriented, are the first k - 1 of
 * step r + 1, so over unitigs every walk is a path over the links of mtg_write_unitig_graph_text. Whatever is indexed, a walk is
 * never wrong, only shorter: a k-mer that occurs more than once is located at its smallest position, which breaks runs and walks.
 * A WALK is a maximal chain of continuing runs; its steps are the runs' (t_record, strand) in order (a ring record taken twice is
 * two steps). Per walk, with K = the sum of n over its runs: q_record, q_start (of the first run), q_end = q_start + K + k - 1,
 * kmers = K, steps, first_step (index of its first step in the step array), path_len = the sum of W(u) over its steps + k - 1,
 * path_start = the offset of the walk's first base in its first step as oriented (t on +, W(u) - (t + n) on -), path_end =
 * path_start + (q_end - q_start). Walks with K < min_kmers are dropped on the device (0 and 1 keep all); the kept walks come in
 * ascending query position and their steps follow each other in the step array, (t_record << 1) | strand each. kmers / valid / found
 * are those of mtg_kmer_index_query. Exact integers, a function of the inputs alone; mtg_tig_index_thread gives the same walks
 * field for field, for every m and bucket_limit. Both die if the index is not locating. Fewer than 2^32 runs per call. */
typedef struct mtg_kmer_walks mtg_kmer_walks;
void mtg_kmer_index_thread(const mtg_kmer_index *ix, const char *seq, const uint64_t *off, uint64_t n, uint64_t min_kmers,
                           uint64_t *kmers, uint64_t *valid, uint64_t *found, /* [n] each */
                           mtg_kmer_walks **out);                             /* mtg_kmer_walks_free */
void mtg_tig_index_thread(const mtg_tig_index *ix, const char *seq, const uint64_t *off, uint64_t n, uint64_t min_kmers,
                          uint64_t *kmers, uint64_t *valid, uint64_t *found, /* [n] each */
                          mtg_kmer_walks **out);                             /* mtg_kmer_walks_free */
uint64_t mtg_kmer_walks_count(const mtg_kmer_walks *walks);
uint64_t mtg_kmer_walks_steps_count(const mtg_kmer_walks *walks);
/* fields[0 .. 9): q_record, q_start, q_end, kmers, steps, first_step, path_len, path_start, path_end -- count entries each; valid
 * until mtg_kmer_walks_free */
void mtg_kmer_walks_arrays(const mtg_kmer_walks *walks, const uint64_t *fields[9]);
const uint64_t *mtg_kmer_walks_steps(const mtg_kmer_walks *walks); /* steps_count entries; valid until mtg_kmer_walks_free */
void mtg_kmer_walks_free(mtg_kmer_walks *walks);                   /* NULL is fine */
/* Of the last mtg_kmer_index_thread / mtg_tig_index_thread on this thread, in ms: {upload (host clock), pack, probe (with the fill of
 * the hit array), runs (flag, scan, emit), walks (flag, scans, emit, compaction)} -- HIP events around the kernels. */
void mtg_last_kmer_thread_times(double out[5]);
void mtg_last_tig_thread_times(double out[5]);
/* The walks as GAF text, one line per walk in the handle's order, written by the host's threads (the walks are on the host by
 * then): query name, query_len[q_record], q_start, q_end, "+", the path (">" + name per + step, "<" + name per - step), path_len,
 * path_start, path_end, matches and alignment length (both q_end - q_start), 255, "cg:Z:{q_end - q_start}=" and "km:i:{kmers}",
 * tab-separated. Name i of a list is the bytes [off[i], off[i + 1]) of its text; segment_names == NULL names index record u by its
 * decimal number, as the S lines of mtg_write_unitig_graph_text do. Dies on a walk or a step beyond the names given. *text_out is
 * malloc'd and 0-terminated (mtg_free). Returns the bytes. */
uint64_t mtg_kmer_walks_gaf(const mtg_kmer_walks *walks, uint64_t n_queries, const char *query_names, const uint64_t *query_name_off,
                            const uint64_t *query_len, uint64_t n_segments, const char *segment_names,
                            const uint64_t *segment_name_off, char **text_out);
/* HOW HEAVY the k-mers of a query are. A WEIGHTED index is built by the two functions below from the sequences and
 * one uint32 per window of them, in window order: a record shorter than k has no window, and the window at global position q of
 * record r has the ordinal (windows of the records before r) + (q - off[r]). n_weights must equal info.occurrences, else the call
 * aborts. weight(class) = weights[ordinal(loc)], loc = the class's smallest window start as mtg_kmer_index_locate defines it: a
 * repeated k-mer takes the weight of its first occurrence, a function of the input alone. The index keeps 4 B per slot more (counted
 * in info.device_bytes). locating = 0: it answers mtg_kmer_index_query and mtg_kmer_index_abundance and aborts on
 * mtg_kmer_index_locate; locating != 0: it is a full locating index as well. Query and locate answer exactly as on an index built
 * without weights. */
mtg_kmer_index *mtg_kmer_index_build_weighted(const char *seq, const uint64_t *off, uint64_t n, uint64_t k, const uint32_t *weights,
                                              uint64_t n_weights, int locating, int device_id);
mtg_kmer_index *mtg_kmer_index_build_weighted_store(const mtg_unitigs *store, uint64_t k, const uint32_t *weights, uint64_t n_weights,
                                                    int locating, int device_id);
int mtg_kmer_index_is_weighted(const mtg_kmer_index *ix);
/* The query of mtg_kmer_index_query (kmers / valid / found as there) plus, for record r over its found windows: sum[r] = the sum of
 * weight(class of the window), in 64 bits; min[r] / max[r] = the smallest / largest such weight; all three 0 when found[r] = 0.
 * per_window (may be NULL; off[n] entries, one per global base position of the query): [p] = the weight of the class of the window
 * that starts at p if that window is valid and found, else 0 -- invalid and absent windows, the last k - 1 positions of a record and
 * records shorter than k. Exact integers, a function of the inputs alone; the index is not changed. An empty query returns at once.
 * Aborts if the index is not weighted. */
void mtg_kmer_index_abundance(const mtg_kmer_index *ix, const char *seq, const uint64_t *off, uint64_t n,
                              uint64_t *kmers, uint64_t *valid, uint64_t *found, /* [n] each */
                              uint64_t *sum, uint32_t *min, uint32_t *max,       /* [n] each */
                              uint32_t *per_window);                             /* nullable, [off[n]] */
/* Of the last mtg_kmer_index_abundance on this thread, in ms: {upload (host clock), pack, probe -- HIP events around the kernels --,
 * download (host clock)}. */
void mtg_last_kmer_abundance_times(double out[4]);
/* WHICH INPUTS carry a k-mer. Every input record r has a colour c(r), 0 <= c(r) < n_colors, 1 <= n_colors <= 64 (a
 * file, a sample, a haplotype). colors(x), for a canonical k-mer x, = the 64-bit mask with bit c(r) for every window of record r
 * whose k-mer is x or rc(x): both strands count, repeats add nothing, and the mask -- like the abundance that decides membership in
 * S_m -- is taken over ALL windows. mtg_compact_unitigs_colored is mtg_compact_unitigs_counted_kmers at the same min_abundance,
 * output for output and byte for byte, plus: *kmer_colors, one mask per k-mer of S_m indexed like *kmer_counts (window order of
 * *out), and *color_stats over the kept k-mers: per_color[c] = those whose mask has bit c; shared[i * 64 + j] = those with bits i and j
 * (symmetric, the diagonal equals per_color; entries with i or j >= n_colors are 0); occupancy[j] = those carried by exactly j colours
 * (occupancy[0] = 0, occupancy[n_colors] the core, occupancy[1] the private ones, the sum distinct_kept). A colour no record has, or
 * whose records are all shorter than k, gives a zero row. Exact integers, a function of the input, min_abundance and the colouring
 * alone. record_colors: n entries; an entry >= n_colors, or n_colors outside 1 .. 64, aborts. */
typedef struct mtg_color_stats {
    uint64_t n_colors;
    uint64_t per_color[64];
    uint64_t occupancy[65];
    uint64_t shared[64 * 64];
} mtg_color_stats;
typedef struct mtg_kmer_colors mtg_kmer_colors;
void mtg_compact_unitigs_colored(const char *data, const uint64_t *offsets, uint64_t n, uint64_t k, uint64_t min_abundance,
                                 const uint8_t *record_colors, uint64_t n_colors, int device_id, mtg_unitigs **out, mtg_compaction *stats,
                                 mtg_abundance *abundance, mtg_abundance_sums **sums, mtg_kmer_counts **kmer_counts,
                                 mtg_kmer_colors **kmer_colors, /* mtg_kmer_colors_free */
                                 mtg_color_stats *color_stats);
void mtg_compact_unitigs_colored_store(const mtg_unitigs *in, uint64_t k, uint64_t min_abundance, const uint8_t *record_colors,
                                       uint64_t n_colors, int device_id, mtg_unitigs **out, mtg_compaction *stats, mtg_abundance *abundance,
                                       mtg_abundance_sums **sums, mtg_kmer_counts **kmer_counts, mtg_kmer_colors **kmer_colors,
                                       mtg_color_stats *color_stats);
uint64_t mtg_kmer_colors_count(const mtg_kmer_colors *colors);        /* the store's k-mers */
const uint64_t *mtg_kmer_colors_array(const mtg_kmer_colors *colors); /* count entries; valid until mtg_kmer_colors_free */
void mtg_kmer_colors_free(mtg_kmer_colors *colors);
/* An index with any of the two payloads. weights (NULL: none) as mtg_kmer_index_build_weighted takes them. colors (NULL: none): one
 * 64-bit mask per window of the sequences, in window order; n_color_words must equal info.occurrences, 1 <= n_colors <= 64 and no
 * mask may have a bit from n_colors on, else the call aborts. color(class) = colors[ordinal(loc)], loc as for the weights: the mask
 * of the class's first occurrence. A coloured index keeps 8 B per slot more. Query, locate and abundance answer exactly as on an
 * index without colours. A payload whose sequences have no window is an array of no entries: any non-NULL pointer and a count of 0. */
mtg_kmer_index *mtg_kmer_index_build_annotated(const char *seq, const uint64_t *off, uint64_t n, uint64_t k, const uint32_t *weights,
                                               uint64_t n_weights, const uint64_t *colors, uint64_t n_color_words, uint64_t n_colors,
                                               int locating, int device_id);
mtg_kmer_index *mtg_kmer_index_build_annotated_store(const mtg_unitigs *store, uint64_t k, const uint32_t *weights, uint64_t n_weights,
                                                     const uint64_t *colors, uint64_t n_color_words, uint64_t n_colors, int locating,
                                                     int device_id);
int mtg_kmer_index_is_colored(const mtg_kmer_index *ix);
uint64_t mtg_kmer_index_n_colors(const mtg_kmer_index *ix); /* 0: not coloured */
/* The query of mtg_kmer_index_query (kmers / valid / found as there) plus per_color (n * n_colors entries, row-major): [r * n_colors +
 * c] = the found windows of record r whose class's mask has bit c. A mask of 0 is a mask: such a
 * window counts as found and touches no column. per_window (may be NULL; off[n] entries): [p] = the mask of the class of the window
 * that starts at p if that window is valid and found, else 0 -- the positions of mtg_kmer_index_abundance's per_window. Exact
 * integers, a function of the inputs alone; the index is not changed. A record has fewer than 2^32 windows. An empty query returns
 * at once. Aborts if the index is not coloured. */
void mtg_kmer_index_colors(const mtg_kmer_index *ix, const char *seq, const uint64_t *off, uint64_t n,
                           uint64_t *kmers, uint64_t *valid, uint64_t *found, /* [n] each */
                           uint32_t *per_color,                               /* [n * n_colors] */
                           uint64_t *per_window);                             /* nullable, [off[n]] */
/* In ms: {the colour statistics kernel of the last mtg_compact_unitigs_colored on this thread (HIP events); of the last
 * mtg_kmer_index_colors: upload (host clock), pack, probe -- HIP events around the kernels --, download (host clock)}. */
void mtg_last_kmer_color_times(double out[5]);
/* The same two answers from the SPARSE index: payloads hung off text positions instead of table slots. weights and
 * colors are exactly what mtg_kmer_index_build_annotated takes (either may be NULL; both NULL gives a plain locating index): one
 * entry per window of the sequences, in window order; the counts must equal info.occurrences, 1 <= n_colors <= 64 and no mask may
 * have a bit from n_colors on, else the call aborts. The index is built in the locating form (mtg_tig_index_is_locating = 1,
 * mtg_tig_index_locate works) and keeps, beside it, the windows before every record (8 B per record) and each payload in one of
 * two layouts: DENSE, one element per window of `width` bytes (weights: the narrowest of 1, 2, 4 that holds the largest weight;
 * masks: the narrowest of 1, 2, 4, 8 that holds n_colors bits), width * windows bytes; or RUNS, the maximal runs of equal
 * consecutive entries, (8 + 4) * runs bytes for weights and (8 + 8) * runs for masks. layout = 0: each payload takes the smaller,
 * dense on a tie; 1: dense; 2: runs; anything else aborts. All of it is counted in info.device_bytes.
 * mtg_tig_index_abundance / mtg_tig_index_colors are mtg_kmer_index_abundance's / mtg_kmer_index_colors' contracts, word for word:
 * for the same sequences, payloads, query and k every output equals that of an annotated mtg_kmer_index, for every m, bucket_limit
 * and layout -- the payload of a k-mer is that of the smallest window start of its class. They abort on an index without that
 * payload. */
mtg_tig_index *mtg_tig_index_build_annotated(const char *seq, const uint64_t *off, uint64_t n, uint64_t k, uint64_t m, uint64_t bucket_limit,
                                             const uint32_t *weights, uint64_t n_weights, const uint64_t *colors, uint64_t n_color_words,
                                             uint64_t n_colors, int layout, int device_id);
mtg_tig_index *mtg_tig_index_build_annotated_store(const mtg_unitigs *store, uint64_t k, uint64_t m, uint64_t bucket_limit,
                                                   const uint32_t *weights, uint64_t n_weights, const uint64_t *colors,
                                                   uint64_t n_color_words, uint64_t n_colors, int layout, int device_id);
int mtg_tig_index_is_weighted(const mtg_tig_index *ix);
int mtg_tig_index_is_colored(const mtg_tig_index *ix);
typedef struct mtg_tig_payload {
    uint64_t layout;       /* 0: the index has no such payload; 1: dense; 2: runs */
    uint64_t width;        /* bytes per element of the dense layout (reported for runs too: what dense would take) */
    uint64_t windows;      /* entries given = info.occurrences */
    uint64_t runs;         /* maximal runs of equal consecutive entries (counted for either layout) */
    uint64_t device_bytes; /* dense: width * windows; runs: (8 + 4 or 8) * runs */
} mtg_tig_payload;
typedef struct mtg_tig_payload_info {
    mtg_tig_payload weights, colors;
    uint64_t n_colors;         /* 0: not coloured */
    uint64_t win_offset_bytes; /* 8 * (records + 1) if there is a payload, else 0 */
} mtg_tig_payload_info;
void mtg_tig_index_get_payload_info(const mtg_tig_index *ix, mtg_tig_payload_info *out);
void mtg_tig_index_abundance(const mtg_tig_index *ix, const char *seq, const uint64_t *off, uint64_t n,
                             uint64_t *kmers, uint64_t *valid, uint64_t *found, /* [n] each */
                             uint64_t *sum, uint32_t *min, uint32_t *max,       /* [n] each */
                             uint32_t *per_window);                             /* nullable, [off[n]] */
void mtg_tig_index_colors(const mtg_tig_index *ix, const char *seq, const uint64_t *off, uint64_t n,
                          uint64_t *kmers, uint64_t *valid, uint64_t *found, /* [n] each */
                          uint32_t *per_color,                               /* [n * n_colors] */
                          uint64_t *per_window);                             /* nullable, [off[n]] */
/* On this thread, in ms: of the last mtg_tig_index_build_annotated, the weights' {upload (host clock), reduce, flag + scan, compact or
 * narrow} then the colours' same four (0 where there is no such payload); of the last mtg_tig_index_abundance or _colors: {upload
 * (host clock), pack, probe (tig_locate_kernel with the fill of the hit array), gather} -- HIP events around the kernels. */
void mtg_last_tig_payload_times(double out[12]);
/* THE INDEX AS A FILE (conventional suffix .mtgx): a sparse index of any kind -- plain, locating, weighted, coloured --
 * written once and reopened without its sequences. A file is little-endian: a fixed header (magic MTGTIGIX, format version 1, a
 * byte-order mark, every field of mtg_tig_index_info but device_bytes, the payload infos, one table entry per section and the
 * header's own digest), a length-prefixed metadata blob that the library stores and returns without reading it, and one section
 * per device array of the index, 4096-aligned, whose bytes are the array as it lies on the device: a load is read -> upload, no
 * rebuild, and info.device_bytes of the loaded index equals the builder's. A file is a function of the index and the blob alone.
 * Every section carries a 64-bit digest computed ON THE GPU over the device array (save: before the download; load: after the upload).
 * mtg_tig_index_save writes to path + ".tmp" and renames at the end; host memory is bounded by the pinned transfer slices, never by
 * the index. 0, or 2 with the reason in err (an error of the output file).
 * mtg_tig_index_load refuses a file that is damaged, truncated, of a later version, or whose arrays break an invariant the probes
 * rely on: NULL, every allocation returned, and err = "<path>: [section <name>:] <check>: ..." (mtg_read_fastq_split's convention,
 * not an abort). The order: header checks on the host before any device allocation (magic, version, byte order, header digest,
 * every section inside the file's length, every count equal to what the info fields imply, k / m / bucket_limit / n_colors inside
 * the build's limits), then every section's digest on the GPU, then the validation kernel. A loaded index is an index like any
 * other: query, locate, abundance, colors, tallies and pseudoaligners take it unchanged.
 * mtg_tig_index_meta: the blob of the file the index was loaded from, or of its last save; empty otherwise. The pointer lives as
 * long as the index and until its next save.
 * mtg_tig_index_file_info: the header checks alone, on the host -- no GPU is touched, it works on a machine without one. meta
 * receives up to meta_cap bytes of the blob, *meta_len its full length. 0, or 2 with err.
 * mtg_last_tig_index_file_times, on this thread, in ms: of the last save {digest kernels, download, write}, of the last load {read,
 * upload, digest kernels, validation kernel}. */
int mtg_tig_index_save(const mtg_tig_index *ix, const char *path, const char *meta_json, uint64_t meta_len, char *err, uint64_t err_len);
mtg_tig_index *mtg_tig_index_load(const char *path, int device_id, char *err, uint64_t err_len);
const char *mtg_tig_index_meta(const mtg_tig_index *ix, uint64_t *len);
int mtg_tig_index_file_info(const char *path, mtg_tig_index_info *info, mtg_tig_payload_info *payload, int *locating, char *meta,
                            uint64_t meta_cap, uint64_t *meta_len, char *err, uint64_t err_len);
void mtg_last_tig_index_file_times(double out[7]);
/* HOW OFTEN OTHER SEQUENCES SEE the indexed k-mers: the opposite question to the probes above. A TALLY belongs to one
 * index -- plain, locating, weighted or coloured --, which must outlive it and which it never changes. It holds one unsigned 64-bit
 * counter per table slot, all 0 at creation: 8 B per slot = 16 B per indexed window, taken from the device arena on the index's
 * device (mtg_kmer_tally_device_bytes = 8 * info.slots) and given back by mtg_kmer_tally_free; mtg_release_device_memory leaves it
 * intact. Several tallies on one index are independent.
 * add: the query of mtg_kmer_index_query (n records of ARBITRARY bytes, the same validity rules; kmers / valid / found as there) and,
 * for every valid window whose canonical k-mer is in the index, tally[class] += 1: repeats inside a record count, both strands fold
 * onto one counter, invalid and absent windows add nothing. Any number of calls accumulate; one call has fewer than 2^40 - 1 bases,
 * as a query, so a 64-bit counter does not overflow and nothing saturates.
 * coverage: ANY sequences may be asked (the indexed ones say how deep the reads cover them); kmers / valid / found as in the query,
 * and for record r over its found windows: covered[r] = those whose class has a tally > 0, sum[r] = the sum of tally(class), max[r] =
 * the largest such tally; all three 0 when found[r] = 0. A k-mer that occurs in several asked windows contributes its class's tally
 * to each of them. per_window (may be NULL; off[n] entries, one per global base position): [p] = the tally of the class of the
 * window that starts at p if that window is valid and found, else 0 -- the positions of mtg_kmer_index_abundance's per_window.
 * reset: every counter 0 again. Exact integers, a function of the index, the sequences added since creation or the last reset, and
 * the sequences asked; integer atomic sums make them independent of launch geometry and arrival order. A null argument or bad
 * offsets abort with the function's name; an empty query returns at once. */
typedef struct mtg_kmer_tally mtg_kmer_tally;
mtg_kmer_tally *mtg_kmer_tally_create(const mtg_kmer_index *ix); /* the index must outlive the tally */
uint64_t mtg_kmer_tally_device_bytes(const mtg_kmer_tally *t);   /* 8 * info.slots */
void mtg_kmer_tally_add(mtg_kmer_tally *t, const char *seq, const uint64_t *off, uint64_t n,
                        uint64_t *kmers, uint64_t *valid, uint64_t *found); /* [n] each */
void mtg_kmer_tally_coverage(const mtg_kmer_tally *t, const char *seq, const uint64_t *off, uint64_t n,
                             uint64_t *kmers, uint64_t *valid, uint64_t *found,       /* [n] each */
                             uint64_t *covered, uint64_t *sum, uint64_t *max,         /* [n] each */
                             uint64_t *per_window);                                   /* nullable, [off[n]] */
/* The same over a store as mtg_read_sequences / mtg_compact_unitigs hand it out: n = mtg_unitigs_count(store). */
void mtg_kmer_tally_add_store(mtg_kmer_tally *t, const mtg_unitigs *store, uint64_t *kmers, uint64_t *valid, uint64_t *found);
void mtg_kmer_tally_coverage_store(const mtg_kmer_tally *t, const mtg_unitigs *store, uint64_t *kmers, uint64_t *valid, uint64_t *found,
                                   uint64_t *covered, uint64_t *sum, uint64_t *max, uint64_t *per_window);
void mtg_kmer_tally_reset(mtg_kmer_tally *t);
void mtg_kmer_tally_free(mtg_kmer_tally *t); /* NULL is fine; any current device */
/* Of the last mtg_kmer_tally_add or mtg_kmer_tally_coverage on this thread, in ms: {upload (host clock), pack, probe -- HIP events
 * around the kernel --, download (host clock)}. */
void mtg_last_kmer_tally_times(double out[4]);
/* The same tally on the SPARSE index: counters hung off text positions instead of table slots. A TIG TALLY belongs to
 * one LOCATING mtg_tig_index (mtg_tig_index_build_locating* or mtg_tig_index_build_annotated*; mtg_tig_tally_create aborts on any
 * other and names mtg_tig_index_build_locating), which must outlive it and which it never changes. It holds one unsigned 64-bit
 * counter per WINDOW ORDINAL of the indexed text (the windows of record 0 from left to right, then record 1's; W = info.occurrences
 * = mtg_tig_tally_windows), all 0 at creation, and the windows before every record (8 B per record + 8) unless the index keeps them
 * already (an annotated index with a payload): mtg_tig_tally_device_bytes = 8 W, plus 8 (records + 1) iff the tally owns those.
 * From the arena on the index's device until mtg_tig_tally_free; mtg_release_device_memory leaves it intact. Several tallies on one
 * index are independent.
 * add / coverage / reset are mtg_kmer_tally_add's / _coverage's / _reset's contracts, word for word: for the same indexed sequences,
 * k, adds and asked sequences every output equals that of a mtg_kmer_tally on a mtg_kmer_index, for every m and bucket_limit. The
 * counter of a class is the one at the ordinal of the smallest window start of the class in the text (what mtg_tig_index_locate
 * reports): mtg_tig_tally_counters copies the W counters out in window order, where a window that is not the first occurrence of its
 * class holds 0 and the sum of all equals the sum of found[] over the adds since creation or the last reset.
 * A null argument or bad offsets abort with the function's name; a query without bases returns at once. */
typedef struct mtg_tig_tally mtg_tig_tally;
mtg_tig_tally *mtg_tig_tally_create(const mtg_tig_index *ix); /* the index must outlive the tally */
uint64_t mtg_tig_tally_device_bytes(const mtg_tig_tally *t);
uint64_t mtg_tig_tally_windows(const mtg_tig_tally *t); /* W */
void mtg_tig_tally_add(mtg_tig_tally *t, const char *seq, const uint64_t *off, uint64_t n,
                       uint64_t *kmers, uint64_t *valid, uint64_t *found); /* [n] each */
void mtg_tig_tally_coverage(const mtg_tig_tally *t, const char *seq, const uint64_t *off, uint64_t n,
                            uint64_t *kmers, uint64_t *valid, uint64_t *found,       /* [n] each */
                            uint64_t *covered, uint64_t *sum, uint64_t *max,         /* [n] each */
                            uint64_t *per_window);                                   /* nullable, [off[n]] */
void mtg_tig_tally_add_store(mtg_tig_tally *t, const mtg_unitigs *store, uint64_t *kmers, uint64_t *valid, uint64_t *found);
void mtg_tig_tally_coverage_store(const mtg_tig_tally *t, const mtg_unitigs *store, uint64_t *kmers, uint64_t *valid, uint64_t *found,
                                  uint64_t *covered, uint64_t *sum, uint64_t *max, uint64_t *per_window);
void mtg_tig_tally_counters(const mtg_tig_tally *t, uint64_t *out); /* [W] */
void mtg_tig_tally_reset(mtg_tig_tally *t);
void mtg_tig_tally_free(mtg_tig_tally *t); /* NULL is fine; any current device */
/* Of the last mtg_tig_tally_add or mtg_tig_tally_coverage on this thread, in ms: {upload (host clock), pack, probe (tig_locate_kernel
 * with the fill of the hit array), the add or the gather -- HIP events around the kernels --, download (host clock)}. */
void mtg_last_tig_tally_times(double out[5]);
/* PSEUDOALIGNMENT against the coloured k-mer set, with EQUIVALENCE CLASSES. A pseudoaligner belongs to one COLOURED
 * index, a mtg_kmer_index (mtg_kmer_index_build_annotated* with colors) or a mtg_tig_index (mtg_tig_index_build_annotated* with
 * colors), which must outlive it and which it never changes. C = n_colors, 1 <= C <= 64; mask(x) is what mtg_kmer_index_colors /
 * mtg_tig_index_colors use: the mask of the class's first occurrence. Exact integers throughout:
 *  - A FRAGMENT is one query record or, with mates, the pair (record r of the reads, record r of the mates); both sets have n records.
 *  - kmers, valid and found of a fragment are mtg_kmer_index_query's columns summed over its one or two records (any byte is
 *    tolerated, a non-ACGT byte costs the windows that cover it, case is folded).
 *  - hits[c] = the found windows of the fragment whose class's mask has bit c: windows, not distinct k-mers -- per_color of
 *    mtg_kmer_index_colors summed over the mates. A class with mask 0 is found and touches no colour.
 *  - params: threshold_permille P in 1 .. 1000; over_valid 0: denom = found, else denom = valid; min_kmers >= 1. NULL params:
 *    {1000, 0, 1}.
 *  - Colour c is ASSIGNED iff denom >= min_kmers, hits[c] > 0 and hits[c] * 1000 >= P * denom, in 64-bit integers. masks[f] = the
 *    bits of the assigned colours. P = 1000 over found: the intersection of the masks of the found windows, the classical
 *    pseudoalignment; over valid it also requires that every valid window was found.
 *  - The EQUIVALENCE CLASSES are the distinct non-zero masks since creation or the last reset; per class mask, fragments (how many
 *    fragments have exactly that mask) and first (the smallest ordinal of such a fragment; ordinals run over every fragment aligned
 *    since creation or reset, across calls). mtg_pseudoaligner_classes returns them ascending by first, in three arrays of the
 *    caller's (mtg_free each; all NULL where there is none).
 *  - totals: fragments, eligible (denom >= min_kmers), assigned (mask != 0), ambiguous (more than one bit), since creation or reset.
 * The per-colour counters never leave the device; a call downloads 4 x 8 B per fragment and the call's classes. The aligner holds no
 * device memory between calls. Aborts with the function's name: a null index, an index without colours, P outside 1 .. 1000,
 * min_kmers = 0, exactly one of mate_seq / mate_off NULL (stores: a mates store with another record count), a fragment with 2^32
 * windows or more, bad offsets. n = 0 returns at once. */
typedef struct mtg_pseudoalign_params { uint64_t threshold_permille, over_valid, min_kmers; } mtg_pseudoalign_params;
typedef struct mtg_pseudoaligner mtg_pseudoaligner;
mtg_pseudoaligner *mtg_pseudoaligner_create(const mtg_kmer_index *ix, const mtg_pseudoalign_params *p);    /* the index outlives it */
mtg_pseudoaligner *mtg_pseudoaligner_create_tig(const mtg_tig_index *ix, const mtg_pseudoalign_params *p); /* the index outlives it */
void mtg_pseudoaligner_align(mtg_pseudoaligner *pa, const char *seq, const uint64_t *off, uint64_t n,
                             const char *mate_seq, const uint64_t *mate_off,                       /* both NULL: single-end */
                             uint64_t *kmers, uint64_t *valid, uint64_t *found, uint64_t *masks); /* [n] each */
void mtg_pseudoaligner_align_store(mtg_pseudoaligner *pa, const mtg_unitigs *reads, const mtg_unitigs *mates, /* mates NULL: single-end */
                                   uint64_t *kmers, uint64_t *valid, uint64_t *found, uint64_t *masks);
uint64_t mtg_pseudoaligner_classes(const mtg_pseudoaligner *pa, uint64_t **mask, uint64_t **fragments, uint64_t **first);
void mtg_pseudoaligner_totals(const mtg_pseudoaligner *pa, uint64_t out[4]); /* fragments, eligible, assigned, ambiguous */
void mtg_pseudoaligner_reset(mtg_pseudoaligner *pa);
void mtg_pseudoaligner_free(mtg_pseudoaligner *pa); /* NULL is fine */
/* Of the last mtg_pseudoaligner_align* on this thread, in ms: {upload (host clock), pack, the colour probe(s), the mask kernel, the
 * dictionary -- HIP events around the kernels --, download (host clock)}. */
void mtg_last_pseudoalign_times(double out[6]);
/* READ CORRECTION against the indexed k-mer set: substitution errors of the query's records are put right where the
 * set says how. Any mtg_kmer_index serves, for any k it takes, and is never changed. Exact integers throughout:
 *  - The SOLID SET is the index's k-mer set: whatever cleaning or threshold formed the indexed sequences decides what is solid.
 *  - A record x[0..n) has the windows i = 0 .. n - k. A base is GOOD iff it is one of ACGTacgt (case is folded, as in
 *    mtg_kmer_index_query). A window is VALID iff all its k bases are good, and PRESENT iff it is valid and its class is in the set.
 *    cover(p) = the valid windows i with max(0, p - k + 1) <= i <= min(p, n - k).
 *  - params: min_solid W >= 1, rounds R in 1 .. 8. NULL params: {4, 2}.
 *  - ONE ROUND; every decision is made against the round's input text, all substitutions are applied together afterwards:
 *      1. p is a CANDIDATE iff x[p] is good, cover(p) is not empty and no window of cover(p) is present.
 *      2. For a candidate and each of the three bases b != x[p] (compared as upper-case ACGT): S(p, b) = the number of windows of
 *         cover(p) that are in the set when x[p] alone is replaced by b.
 *      3. best = max over b of S(p, b), need = min(W, |cover(p)|). best < need: nothing happens. Two or more b attain best (and
 *         best >= need): p is AMBIGUOUS and nothing happens. Otherwise x[p] is substituted by that b.
 *  - Round r + 1 runs on round r's output. A substituted position is covered by a present window from then on and is never a
 *    candidate again, provided no other substitution of the same round lies within k - 1 of it (two such are each scored against
 *    the other's old base; a window that holds both may be solid with neither pair, and the position may be substituted again). A
 *    round that substitutes nothing anywhere ends the rounds: every later one would be identical.
 *  - Per record: kmers, valid, found = mtg_kmer_index_query's columns on the input; found_after = found on the final text;
 *    candidates = the candidates of round 1; ambiguous = the ambiguous positions of round R; corrected = the positions substituted
 *    over all rounds: those whose base in the final text is not the input's.
 *  - Per call: the substitutions as *positions (index into the concatenated query data, ascending, each once) and *bases ('A', 'C',
 *    'G' or 'T', the base of the final text; the caller keeps the case of the letter it replaces), *n_substitutions entries each,
 *    malloc'd (mtg_free each; both NULL where there is none); round_corrected[r] = the substitutions made in round r + 1, 0 for
 *    the rounds not run (their sum exceeds *n_substitutions only where a position was substituted twice).
 * The bit arrays, the candidates and the text never leave the device; a call downloads 5 x 8 B per record and 9 B per substitution
 * and holds no device memory afterwards. Aborts with the function's name: min_solid = 0, rounds outside 1 .. 8, a null argument, bad
 * offsets, 2^40 - 1 bases or more. n = 0 returns at once. The cost of a candidate grows with k^2 for k >= 32. */
typedef struct mtg_correct_params { uint32_t min_solid, rounds; } mtg_correct_params;
void mtg_kmer_index_correct(const mtg_kmer_index *ix, const char *seq, const uint64_t *off, uint64_t n, const mtg_correct_params *params,
                            uint64_t *kmers, uint64_t *valid, uint64_t *found, uint64_t *found_after, /* [n] each */
                            uint64_t *candidates, uint64_t *ambiguous, uint64_t *corrected,           /* [n] each */
                            uint64_t **positions, uint8_t **bases, uint64_t *n_substitutions, uint64_t round_corrected[8]);
void mtg_kmer_index_correct_store(const mtg_kmer_index *ix, const mtg_unitigs *reads, const mtg_correct_params *params,
                                  uint64_t *kmers, uint64_t *valid, uint64_t *found, uint64_t *found_after,
                                  uint64_t *candidates, uint64_t *ambiguous, uint64_t *corrected,
                                  uint64_t **positions, uint8_t **bases, uint64_t *n_substitutions, uint64_t round_corrected[8]);
/* Of the last mtg_kmer_index_correct* on this thread, in ms: {upload (host clock), pack, the query passes, flag and compaction, the
 * evaluation, apply -- HIP events around the kernels --, download (host clock), the whole call (host clock)}. */
void mtg_last_kmer_correct_times(double out[8]);
/* MONOCHROMATIC UNITIGS and COLOUR CLASSES. mtg_compact_unitigs_colored_classes is mtg_compact_unitigs_colored plus
 * *classes, the dictionary of the output store's masks. Number the windows of *out i = 0 .. N - 1 in window order (the indexing of
 * *kmer_colors). A RUN is a maximal stretch of consecutive windows of ONE unitig with equal masks. The classes are the distinct masks,
 * numbered 0, 1, ... in the order of the first window that shows them; per class c: masks[c], kmers[c] (the windows with that mask; the
 * sum is N), runs[c] (the sum is the number of runs), first[c] (the first window that shows it: strictly increasing in c); per
 * window: kmer_class[i], so masks[kmer_class[i]] = kmer_colors[i].
 * split = 0: *out, *stats, *abundance, *sums, *kmer_counts, *kmer_colors and *color_stats are mtg_compact_unitigs_colored's, byte for
 * byte. split = 1: the compaction's rule for a passable node gains a clause -- the k-mer that enters the node and the k-mer that
 * leaves it have equal masks -- so every unitig of *out is MONOCHROMATIC (one run; the sum of runs is stats->unitigs); a closed walk
 * whose k-mers do not share one mask opens into chains, each with its own leader, direction and place in the order. *out, *stats,
 * *sums, *kmer_counts and *kmer_colors then describe the split store; the scalars and the spectrum of *abundance and all of *color_stats
 * are functions of the k-mer set and equal the unsplit call's. With one colour, or wherever no passable node separates two masks, the
 * split store is the unsplit one. Exact integers that depend on the input, min_abundance, the colours and split alone. split outside
 * {0, 1} or a null out-pointer aborts; the other arguments as for mtg_compact_unitigs_colored. */
typedef struct mtg_color_classes mtg_color_classes;
void mtg_compact_unitigs_colored_classes(const char *data, const uint64_t *offsets, uint64_t n, uint64_t k, uint64_t min_abundance,
                                         const uint8_t *record_colors, uint64_t n_colors, int split, int device_id, mtg_unitigs **out,
                                         mtg_compaction *stats, mtg_abundance *abundance, mtg_abundance_sums **sums,
                                         mtg_kmer_counts **kmer_counts, mtg_kmer_colors **kmer_colors, mtg_color_stats *color_stats,
                                         mtg_color_classes **classes /* mtg_color_classes_free */);
void mtg_compact_unitigs_colored_classes_store(const mtg_unitigs *in, uint64_t k, uint64_t min_abundance, const uint8_t *record_colors,
                                               uint64_t n_colors, int split, int device_id, mtg_unitigs **out, mtg_compaction *stats,
                                               mtg_abundance *abundance, mtg_abundance_sums **sums, mtg_kmer_counts **kmer_counts,
                                               mtg_kmer_colors **kmer_colors, mtg_color_stats *color_stats, mtg_color_classes **classes);
/* The same dictionary for masks handed in: kmer_colors, n masks in window order of a store whose unitig u has unitig_kmers[u] k-mers
 * (n_unitigs entries >= 1 that sum to n; fewer than 2^31 - 1 k-mers). A mask of 0, or lengths that do not fit, abort. What
 * mtg_compact_unitigs_colored_classes returns equals this call on its own *kmer_colors and unitig lengths. */
void mtg_color_classes_build(const uint64_t *kmer_colors, uint64_t n, const uint64_t *unitig_kmers, uint64_t n_unitigs, int device_id,
                             mtg_color_classes **classes);
uint64_t mtg_color_classes_count(const mtg_color_classes *classes);        /* the classes */
const uint64_t *mtg_color_classes_masks(const mtg_color_classes *classes); /* count entries each; valid until mtg_color_classes_free */
const uint64_t *mtg_color_classes_kmers(const mtg_color_classes *classes);
const uint64_t *mtg_color_classes_runs(const mtg_color_classes *classes);
const uint64_t *mtg_color_classes_first(const mtg_color_classes *classes);
uint64_t mtg_color_classes_kmer_class_count(const mtg_color_classes *classes); /* the store's k-mers */
const uint32_t *mtg_color_classes_kmer_class(const mtg_color_classes *classes);
void mtg_color_classes_free(mtg_color_classes *classes);
/* In ms, of the last mtg_compact_unitigs_colored_classes on this thread: {run heads, class table, class ids, counts -- HIP events
 * around the kernels --, download (host clock)}. */
void mtg_last_color_class_times(double out[5]);
/* {the classes the counts kernel keeps in LDS, its largest grid, its block}: what an input must exceed to reach the kernel's other paths. */
void mtg_color_class_limits(uint64_t out[3]);
/* TIP CLIPPING and ISOLATED UNITIGS. mtg_compact_unitigs_cleaned is mtg_compact_unitigs_colored_classes over a k-mer set
 * T that starts as S_m and shrinks in rounds. With the oriented edges of G(T), an OPEN walk W = e_1 .. e_n of the contract over T
 * has two ends: its head node (the suffix of e_n) and the head node of its mirror walk (the reverse complement of the prefix of
 * e_1). For an end with head node v: beyond = |out(v)|, beside = |into(v)| - 1; at a self-mirror node beyond = beside = |out(v)| - 1
 * (our own mirror leaves v). The end is FREE iff beyond = beside = 0, ANCHORED iff beside >= 1, THROUGH otherwise. W is a TIP iff
 * n < tip_kmers, one end is free and the other anchored; ISOLATED iff n < isolated_kmers and both ends are free. Closed walks are
 * never removed. A ROUND decides all walks of T on one snapshot and removes the k-mers of every tip and isolated walk; rounds repeat
 * on the unitigs of the new T until one removes nothing or `rounds` have run. The result is the contract of the lower rungs over the
 * final T -- creators, readings, abundances and masks still taken over ALL windows. With split = 1 the decisions are taken on the
 * unsplit unitigs of T; only the final pass splits.
 * *stats, *sums, *kmer_counts, *kmer_colors, *color_stats and *classes describe the final store; *abundance keeps its meaning
 * (distinct_kept = |S_m|, kept_occurrences over S_m), so the sum of *sums is kept_occurrences - removed_occurrences.
 * Null out-pointers select a lower rung: classes (then split must be 0); kmer_colors and color_stats (then record_colors is not read);
 * kmer_counts; abundance and sums (then min_abundance must be 1 and removed_occurrences is 0). params == NULL or cleaning == NULL, or
 * both lengths 0, cleans nothing: the call then runs the kernels of the rung it selects and returns that rung's bytes. rounds outside
 * 1 .. 64 aborts. Exact integers that depend on the input and the parameters alone. */
typedef struct mtg_cleaning_params {
    uint64_t tip_kmers;      /* a tip has fewer k-mers than this; 0 = no tip clipping */
    uint64_t isolated_kmers; /* an isolated unitig has fewer k-mers than this; 0 = keep them */
    uint64_t rounds;         /* 1 .. 64 */
} mtg_cleaning_params;
typedef struct mtg_cleaning {
    uint64_t rounds_run;           /* the decision rounds that ran, the one that removed nothing included */
    uint64_t tips, tip_kmers;      /* walks removed as tips over all rounds, and their k-mers */
    uint64_t isolated, isolated_kmers;
    uint64_t removed_occurrences;  /* the sum of the removed k-mers' abundances */
} mtg_cleaning;
void mtg_compact_unitigs_cleaned(const char *data, const uint64_t *offsets, uint64_t n, uint64_t k, uint64_t min_abundance,
                                 const uint8_t *record_colors, uint64_t n_colors, int split, const mtg_cleaning_params *params, int device_id,
                                 mtg_unitigs **out, mtg_compaction *stats, mtg_abundance *abundance, mtg_abundance_sums **sums,
                                 mtg_kmer_counts **kmer_counts, mtg_kmer_colors **kmer_colors, mtg_color_stats *color_stats,
                                 mtg_color_classes **classes, mtg_cleaning *cleaning);
void mtg_compact_unitigs_cleaned_store(const mtg_unitigs *in, uint64_t k, uint64_t min_abundance, const uint8_t *record_colors,
                                       uint64_t n_colors, int split, const mtg_cleaning_params *params, int device_id, mtg_unitigs **out,
                                       mtg_compaction *stats, mtg_abundance *abundance, mtg_abundance_sums **sums,
                                       mtg_kmer_counts **kmer_counts, mtg_kmer_colors **kmer_colors, mtg_color_stats *color_stats,
                                       mtg_color_classes **classes, mtg_cleaning *cleaning);
/* Of the last compaction on this thread: {ms of the decision and removal kernels over all rounds (HIP events), the rounds run}.
 * mtg_last_compact_times' nodes and rank phases include every round's. */
void mtg_last_clean_times(double out[2]);
/* BUBBLE POPPING. mtg_compact_unitigs_simplified is mtg_compact_unitigs_cleaned whose rounds also pop the weaker arms
 * of simple bubbles. Over the current set T, an OPEN walk W = e_1 .. e_n has the tail node u (the prefix of e_1 as read) and the head
 * node v (the suffix of e_n); its mirror runs from rc(v) to rc(u) and is the same arm. W is a CANDIDATE ARM iff n < max_arm_kmers,
 * neither u nor v is its own reverse complement, u != v and u != rc(v). The candidate arms with one (u, v) are a BUNDLE. Arm a is
 * BETTER than arm b iff sum_a n_b > sum_b n_a (sum: the abundances of the arm's k-mers), on equality the one with the smaller
 * min(creator of e_1's k-mer, creator of e_n's k-mer). Every arm a other than the bundle's best B is POPPED iff
 * sum_B n_a >= min_ratio sum_a n_B (exact integers; the right side is taken in 128 bits). A longer walk between u and v is in no
 * bundle, closed walks are never touched, and an arm is never a tip or isolated: a round decides all three on one snapshot and
 * removes their k-mers together; rounds repeat until one removes nothing or params->rounds have run.
 * The arguments and the rungs are those of mtg_compact_unitigs_cleaned; everything returned describes the final store, so the sum
 * of *sums is kept_occurrences - cleaning->removed_occurrences - bubbles->removed_occurrences. bubble_params == NULL, bubbles == NULL or
 * max_arm_kmers 0 pops nothing: the call then runs the kernels of the cleaned call and nothing else. With max_arm_kmers > 0 the call
 * must be counted (abundance and sums given) and params and cleaning must be given (params carries the rounds; both of its lengths
 * may be 0), else it aborts; so does min_ratio outside 1 .. 255. */
typedef struct mtg_bubble_params {
    uint64_t max_arm_kmers; /* an arm has fewer k-mers than this; 0 = no popping */
    uint64_t min_ratio;     /* 1 .. 255: the best arm's mean abundance is at least this many times the popped arm's */
} mtg_bubble_params;
typedef struct mtg_bubbles {
    uint64_t arms;                /* arms popped over all rounds */
    uint64_t arm_kmers;           /* their k-mers */
    uint64_t removed_occurrences; /* the sum of those k-mers' abundances */
} mtg_bubbles;
void mtg_compact_unitigs_simplified(const char *data, const uint64_t *offsets, uint64_t n, uint64_t k, uint64_t min_abundance,
                                    const uint8_t *record_colors, uint64_t n_colors, int split, const mtg_cleaning_params *params,
                                    const mtg_bubble_params *bubble_params, int device_id, mtg_unitigs **out, mtg_compaction *stats,
                                    mtg_abundance *abundance, mtg_abundance_sums **sums, mtg_kmer_counts **kmer_counts,
                                    mtg_kmer_colors **kmer_colors, mtg_color_stats *color_stats, mtg_color_classes **classes,
                                    mtg_cleaning *cleaning, mtg_bubbles *bubbles);
void mtg_compact_unitigs_simplified_store(const mtg_unitigs *in, uint64_t k, uint64_t min_abundance, const uint8_t *record_colors,
                                          uint64_t n_colors, int split, const mtg_cleaning_params *params,
                                          const mtg_bubble_params *bubble_params, int device_id, mtg_unitigs **out, mtg_compaction *stats,
                                          mtg_abundance *abundance, mtg_abundance_sums **sums, mtg_kmer_counts **kmer_counts,
                                          mtg_kmer_colors **kmer_colors, mtg_color_stats *color_stats, mtg_color_classes **classes,
                                          mtg_cleaning *cleaning, mtg_bubbles *bubbles);
/* Of the last compaction on this thread: {ms of the list, sums, choose and verdict kernels over all rounds (HIP events; 0 where
 * nothing was to be popped)}. mtg_last_clean_times leaves them out. */
void mtg_last_bubble_times(double out[1]);
/* K-MER SELECTION. mtg_compact_unitigs_selected is mtg_compact_unitigs_simplified over the k-mers of S_m that pass a
 * selection by their colour sets and against FILTER RECORDS, a second sequence store that is looked up in the k-mer table and never
 * inserted: a filter window creates, counts and colours nothing. Abundance(x), colors(x), creator(x), reading(x) and S_m are those of
 * the main records alone. Filter record r has the role filter_roles[r]: 0 = subtract, 1 = intersect; its windows follow the rules of
 * the main records (either case, either strand, a record shorter than k has no window; the caller cuts the records at whatever is
 * outside ACGT). sub(x) = the windows of subtract records whose k-mer is x or rc(x) (a palindromic window counts once), int(x) the
 * same over all intersect records. x in S_m is SELECTED iff it passes, in this order,
 *   1 forbid     colors(x) & forbid == 0
 *   2 require    colors(x) & require == require
 *   3 carriers   min_colors <= popcount(colors(x)) <= max_colors
 *   4 subtract   sub(x) < subtract_min_abundance     (only where a subtract record is given)
 *   5 intersect  int(x) >= intersect_min_abundance   (only where an intersect record is given)
 * and a rejected k-mer is counted under the first rule it fails. The selected set S_sel takes the place of S_m in everything behind
 * it: nodes, successors (split or not), the cleaning rounds, bubbles, the unitigs, sums, ordered counts, masks and classes; the order
 * and the orientation of the unitigs follow the creators and readings of the main windows.
 * *stats, *sums, *kmer_counts, *kmer_colors, *classes, *cleaning and *bubbles describe the output store. *abundance keeps its meaning
 * (distinct_kept = |S_m|), and so does *color_stats: in a selected call it is taken over S_m, also where the call cleans -- the matrix
 * and its occupancy row are how a carrier threshold is chosen, as the spectrum is for min_abundance. With forbid = require = 0,
 * min_colors = 0, max_colors = 64 and no filter record every k-mer is selected and store, sums, counts, masks and classes are those of
 * the call without a selection, byte for byte. An empty S_sel is a result: the store is empty, the statistics are filled.
 * selection_params == NULL or selection == NULL selects nothing: the call then runs the kernels of mtg_compact_unitigs_simplified and
 * nothing else. A selection needs the abundance and sums out-pointers (min_abundance may be 1), and the colours' out-pointers if a
 * colour rule is set (forbid or require != 0, min_colors > 0 or max_colors < 64). Aborts, by name and before any device call: a bit
 * of require or forbid at or beyond n_colors, require & forbid != 0, min_colors > max_colors, max_colors > 64, either filter
 * abundance < 1, a role other than 0 or 1, 2^32 or more filter windows of one role. Exact integers that depend on the inputs and the
 * parameters alone. */
typedef struct mtg_selection_params {
    uint64_t require, forbid;         /* colour masks */
    uint64_t min_colors, max_colors;  /* bounds on the carriers; 0 and 64 bound nothing */
    uint64_t subtract_min_abundance;  /* A >= 1: a k-mer goes iff sub(x) >= A */
    uint64_t intersect_min_abundance; /* B >= 1: a k-mer stays iff int(x) >= B */
} mtg_selection_params;
typedef struct mtg_selection {
    uint64_t input_kmers;                    /* |S_m| */
    uint64_t rejected_forbid, rejected_require, rejected_carriers, rejected_subtract, rejected_intersect; /* by the first rule failed */
    uint64_t selected, selected_occurrences; /* |S_sel| and the sum of its abundances: the five counts + selected == input_kmers */
    uint64_t subtract_windows, intersect_windows; /* the windows of the filter records, by role */
    uint64_t subtract_hits, intersect_hits;  /* those whose class is in the k-mer table at all (of any abundance) */
    uint64_t per_color_selected[64];         /* the selected k-mers with bit c (zeros in a call without colours) */
} mtg_selection;
void mtg_compact_unitigs_selected(const char *data, const uint64_t *offsets, uint64_t n, uint64_t k, uint64_t min_abundance,
                                  const uint8_t *record_colors, uint64_t n_colors, int split, const mtg_cleaning_params *params,
                                  const mtg_bubble_params *bubble_params, const mtg_selection_params *selection_params,
                                  const char *filter_data, const uint64_t *filter_offsets, const uint8_t *filter_roles, uint64_t filter_n,
                                  int device_id, mtg_unitigs **out, mtg_compaction *stats, mtg_abundance *abundance, mtg_abundance_sums **sums,
                                  mtg_kmer_counts **kmer_counts, mtg_kmer_colors **kmer_colors, mtg_color_stats *color_stats,
                                  mtg_color_classes **classes, mtg_cleaning *cleaning, mtg_bubbles *bubbles, mtg_selection *selection);
void mtg_compact_unitigs_selected_store(const mtg_unitigs *in, uint64_t k, uint64_t min_abundance, const uint8_t *record_colors,
                                        uint64_t n_colors, int split, const mtg_cleaning_params *params,
                                        const mtg_bubble_params *bubble_params, const mtg_selection_params *selection_params,
                                        const char *filter_data, const uint64_t *filter_offsets, const uint8_t *filter_roles,
                                        uint64_t filter_n, int device_id, mtg_unitigs **out, mtg_compaction *stats, mtg_abundance *abundance,
                                        mtg_abundance_sums **sums, mtg_kmer_counts **kmer_counts, mtg_kmer_colors **kmer_colors,
                                        mtg_color_stats *color_stats, mtg_color_classes **classes, mtg_cleaning *cleaning,
                                        mtg_bubbles *bubbles, mtg_selection *selection);
/* Of the last compaction on this thread, in ms by HIP events: {the filter probe kernel, the selection (the keep kernel, the scan and
 * the move)}; 0 in a call without a selection. mtg_last_compact_times' ids phase leaves the probe out. */
void mtg_last_select_times(double out[2]);
/* mtg_read_sequences without an alphabet rule: every byte of a sequence line is kept as it is (`N`, IUPAC codes, lower case), for
 * the queries of a k-mer index. *names_out = the record names as a second store with the same accessors: the header text behind `>`
 * up to the first white space. */
void mtg_read_sequences_named(const char *path, mtg_unitigs **seqs_out, mtg_unitigs **names_out);
/* FASTQ reads, read on GPU `device_id` (fastq_device.hip; there is no CPU path). Strict four-line FASTQ, optionally
 * `.gz`: the text is a sequence of lines ended by "\n", one "\r" before it belongs to the line end, a missing final "\n" is
 * tolerated, and so are empty lines behind the last record. Record r is lines 4r .. 4r+3: the first begins with `@`, the third with
 * `+` (what follows it is ignored), the second (bases) and the fourth (qualities, bytes '!' .. '~') have the same length, which may be
 * 0. The kind of a line is its index mod 4 and nothing else. Base j of a record is good when it is one of ACGTacgt and
 * quality[j] - 33 >= min_base_quality (0 .. 93; 0 keeps every ACGT base).
 * mtg_read_fastq_split: the maximal runs of good bases of every record, upper-cased, in file order, as the records of an ordinary
 * store -- mtg_read_sequences_split's rule with "not good" for "not ACGT"; with min_base_quality = 0 store and pieces_cut are what
 * that reader gives for the same reads written as FASTA. mtg_read_fastq_named: the records whole with their characters as they are,
 * a base whose quality is below the threshold replaced by `N`, plus the names (the header text behind `@` up to the first white
 * space) -- mtg_read_sequences_named for FASTQ; there pieces = records and bases_kept = bases.
 * Both return 0 and the store(s), or non-zero when the FILE is malformed: no store is allocated and err (may be NULL) holds
 * "<path>: record <0-based r> (line <1-based l>): <reason>" for the smallest record that breaks a rule and, in it, the first rule
 * broken in the order above; a line count that is no multiple of 4 is reported for the incomplete record with the file's last line.
 * The process goes on. Null arguments, an unreadable path and min_base_quality > 93 abort as in the other readers. */
typedef struct mtg_fastq_stats {
    uint64_t records, bases;  /* records read; the characters of their sequence lines */
    uint64_t non_acgt_bases;  /* bases outside ACGTacgt */
    uint64_t masked_bases;    /* ACGT bases whose quality is below the threshold */
    uint64_t pieces;          /* records of the store */
    uint64_t bases_kept;      /* characters of the store */
    uint64_t pieces_cut;      /* runs of bases that are not good, counted as mtg_read_sequences_split counts its runs */
    uint64_t tile_bytes;      /* text bytes per block of the scan kernels (for tests that place data across tile edges) */
} mtg_fastq_stats;
int mtg_read_fastq_split(const char *path, uint64_t min_base_quality, int device_id, mtg_unitigs **store_out, mtg_fastq_stats *stats,
                         char *err, uint64_t err_capacity);
int mtg_read_fastq_named(const char *path, uint64_t min_base_quality, int device_id, mtg_unitigs **seqs_out, mtg_unitigs **names_out,
                         mtg_fastq_stats *stats, char *err, uint64_t err_capacity);
/* What the first byte that is no line end says about a sequence file (optionally `.gz`): 0 = there is none, 1 = FASTA (`>`),
 * 2 = FASTQ (`@`), -1 = anything else. The file name plays no part. Aborts on an unreadable path. */
int mtg_sequence_file_format(const char *path);
/* Of the last mtg_read_fastq_* on this thread, in ms: {read + inflate (host clock), upload (host clock), lines + check, pieces -- HIP
 * events around the kernels --, download with the name slicing (host clock), the whole call (host clock)}. */
void mtg_last_fastq_times(double out[6]);
uint64_t mtg_unitigs_count(const mtg_unitigs *u);
const char *mtg_unitigs_data(const mtg_unitigs *u);        /* concatenated ASCII sequences */
const uint64_t *mtg_unitigs_offsets(const mtg_unitigs *u); /* count + 1 offsets into data */
/* A new store of the records i of `u` with keep[i] != 0 (count bytes), in their order; host only. Free with mtg_unitigs_free. */
void mtg_unitigs_select(const mtg_unitigs *u, const uint8_t *keep, mtg_unitigs **out);
void mtg_unitigs_free(mtg_unitigs *u);
/* Spells `tigs` (mtg_write_walks_fasta) into a file; a ".gz" suffix selects gzip at compression_level 0-9
 * (bin.rs:203, :442-446; pass 6 for the reference's default). Returns the uncompressed byte count. */
uint64_t mtg_write_tigs_fasta_file(const mtg_graph *g, const mtg_walks *tigs, uint64_t k, const mtg_unitigs *unitigs,
                                   const char *path, int compression_level);
/* The same tigs as GFA1 text (bin.rs:667-818): header line (`header`, e.g. the one read from a GFA input, or NULL for
 * "H\tKL:Z:{k}"), then one "S\t{i+1}\t{sequence}" record per tig. */
uint64_t mtg_write_walks_gfa(const mtg_graph *g, uint64_t n_walks, const uint64_t *limits, const uint32_t *edges, uint64_t k,
                             const char *unitig_seqs, const uint64_t *seq_offsets, const char *header, char **gfa_out);
uint64_t mtg_write_tigs_gfa_file(const mtg_graph *g, const mtg_walks *tigs, uint64_t k, const mtg_unitigs *unitigs,
                                 const char *header, const char *path, int compression_level);
/* Both file writers with the GPU to spell on named explicitly (mtg_config.device_ids[0] of the run that made the tigs): gfa == 0
 * writes FASTA, else GFA with `gfa_header` or "H\tKL:Z:{k}". The two functions above spell on GPU 0. */
uint64_t mtg_write_tigs_text_file_device(const mtg_graph *g, const mtg_walks *tigs, uint64_t k, const mtg_unitigs *unitigs, int gfa,
                                         const char *gfa_header, const char *path, int compression_level, int device_id);
/* The same text (FASTA when gfa == 0, else GFA with `gfa_header` or "H\tKL:Z:{k}") spelled ON THE GPU `device_id`: the unitig
 * store is packed to 2 bits per base on the device and one kernel writes the characters at prefix-summed offsets. Byte-identical to
 * mtg_write_walks_fasta / _gfa for upper-case ACGT input (lower case is accepted and written upper case; any other character
 * aborts, like the reference's DnaAlphabet store). mtg_write_tigs_fasta_file / _gfa_file use this path whenever a GPU is present. */
uint64_t mtg_write_walks_text_device(const mtg_graph *g, uint64_t n_walks, const uint64_t *limits, const uint32_t *edges, uint64_t k,
                                     const char *unitig_seqs, const uint64_t *seq_offsets, int gfa, const char *gfa_header, int device_id,
                                     char **text_out);
double mtg_last_spell_kernel_ms(void); /* HIP-event time of the last spelling kernel on this thread */
uint64_t mtg_last_spell_bytes(void);   /* HBM bytes it moved (text written + packed bases + per-position metadata) */
/* ---- the unitig graph with its links, made on the GPU ------------------------------------------------------
 * Unitig u (record u of the store) has two orientations: (u,+) is edge 2u, (u,-) is edge 2u + 1. Oriented unitig o links to o' iff
 * from(edge o') == to(edge o); only the original edges count, so a tig computation that appended dummy edges changes nothing.
 * mtg_unitig_links: *link_off gets 2U + 1 offsets, *link_to the target edge ids -- those of o are link_to[link_off[o] ..
 * link_off[o + 1]), ascending. Both arrays are released with mtg_free. Returns the number of links. Aborts without a GPU. */
uint64_t mtg_unitig_links(const mtg_graph *g, int device_id, uint64_t **link_off, uint32_t **link_to);
/* The graph as text, written by one kernel on GPU `device_id`. gfa == 0: BCALM2/GGCAT FASTA, per unitig
 * ">{u} LN:i:{len} KC:i:{KC} km:f:{km}" + " L:{+-}:{v}:{+-}" per link + "\n{sequence}\n" -- the links of (u,+) before those of
 * (u,-), each ascending by target edge --; else GFA1: "H\tVN:Z:1.0\tKL:Z:{k}", then per unitig
 * "S\t{u}\t{sequence}\tLN:i:{len}\tKC:i:{KC}\tkm:f:{km}" followed by its links "L\t{u}\t{+-}\t{v}\t{+-}\t{k-1}M".
 * unitig_kc: the abundance sum of every unitig, or NULL for its number of k-mers; km = KC / k-mers with one decimal, rounded half up
 * in integers. n_unitigs sequences of at least k bases each (ACGT, either case; written upper case), as many as the graph has
 * unitigs. *text_out is released with mtg_free. Returns the bytes. Aborts without a GPU. */
uint64_t mtg_write_unitig_graph_text(const mtg_graph *g, const char *unitig_seqs, const uint64_t *seq_offsets, uint64_t n_unitigs,
                                     uint64_t k, const uint64_t *unitig_kc, int gfa, int device_id, char **text_out);
/* The same text into a file; a ".gz" suffix selects gzip at compression_level 0-9. Returns the uncompressed byte count. */
uint64_t mtg_write_unitig_graph_file(const mtg_graph *g, const char *unitig_seqs, const uint64_t *seq_offsets, uint64_t n_unitigs,
                                     uint64_t k, const uint64_t *unitig_kc, int gfa, int device_id, const char *path,
                                     int compression_level);
/* Of the last of the three calls above on this thread: {upload (host clock, ms), link kernels, scans of the text, text kernel -- HIP
 * events, ms --, download (host clock, ms), links, bytes of the text, bytes the text kernel must move at the least, peak of the
 * device arena's live bytes}. */
void mtg_last_unitig_graph_times(double out[9]);
/* ---- the connected components of the unitig graph, on the GPU ------------------------------------------------
 * Unitigs u and v are adjacent iff some orientation of the one links to some orientation of the other by the rule of
 * mtg_unitig_links (from(edge o') == to(edge o), original edges only); a component is a class of the closure of that: connectivity
 * over LINKS, not over shared nodes. Components are numbered 0 .. C - 1 by their smallest unitig, ascending. One entry per
 * component: its smallest unitig, its unitigs, the sums of unitig_kmers and of unitig_kc over them, its link entries (those of
 * mtg_unitig_links whose source orientation lies in it), its orientations without a link, and its orientations whose number of links
 * is not 1 -- none: every orientation has exactly one way on and the component is a closed ring. */
typedef struct mtg_component_arrays {
    uint32_t *first_unitig;
    uint32_t *unitigs;
    uint64_t *kmers;
    uint64_t *abundance;
    uint64_t *links;
    uint32_t *dead_ends;
    uint32_t *irregular;
} mtg_component_arrays;
/* unitig_kmers: the number of k-mers of every unitig (U values); unitig_kc: their abundance sums, or NULL for the number of k-mers.
 * *component_of gets U component numbers; it and the seven arrays of *components are released with mtg_free. Fewer than 2^31
 * unitigs. Returns C. The link lists are not built. Aborts without a GPU. */
uint64_t mtg_unitig_components(const mtg_graph *g, const uint64_t *unitig_kmers, const uint64_t *unitig_kc, int device_id,
                               uint32_t **component_of, mtg_component_arrays *components);
/* Of the last mtg_unitig_components on this thread: {upload (host clock, ms), label kernels, statistics kernel -- HIP events, ms --,
 * download (host clock, ms), components, unitigs, peak of the device arena's live bytes, and the parts of the label kernels' time:
 * rep / degree, the unions, flatten + scan + numbers}. The union-find's retries are not counted. */
void mtg_last_unitig_components_times(double out[10]);
/* Measurement switch: 0 sends every unitig's statistics to its component's counters by itself; the default (1) aggregates the lanes
 * of a wave that share a component first. The results are the same. */
void mtg_set_unitig_components_aggregation(int on);
/* ---- the bubbles of the unitig graph as variant calls, on the GPU ----------------------------------------------
 * Oriented unitig 2u is record u as written, 2u + 1 its reverse complement; x = from(edge 2u) and y = to(edge 2u) are its end nodes
 * and n(u) its k-mers. Unitig u is a candidate arm iff n(u) < max_arm_kmers and it has no self-mirror end (x = mirror(x) or
 * y = mirror(y)), is no loop (x = y) and no hairpin (x = mirror(y)). Its key is the smaller of the node pairs (x, y) and
 * (mirror(y), mirror(x)); the candidates of one key are a bundle, and a bundle of two or more arms is a bubble. Arm a is better than b
 * iff unitig_kc[a] n(b) > unitig_kc[b] n(a), taken in 128 bits, on equality the smaller unitig; the best arm is the reference arm r.
 * Bubbles are numbered by their smallest unitig, ascending; the arms of bubble b are entries arm_off[b] .. arm_off[b + 1] - 1, r
 * first, the others ascending by unitig. arm_strand: 0 where the arm runs between the same two nodes as record r as written, 1 where
 * its reverse complement does; the allele is the oriented unitig 2 arm_unitig + arm_strand. arm_kmers = n, arm_abundance = unitig_kc
 * (n without it). For every other arm against R = record r: suffix = the longest common suffix of R and the allele, at most the
 * shorter length; prefix = the longest common prefix, at most the shorter length less the suffix (so indels are left-aligned);
 * ref = R[prefix, |R| - suffix), alt likewise; differences = the positions at which ref and alt differ where their lengths agree,
 * else 0. All three are 0 for arm 0. carried[arm * n_colors + c] = the arm's k-mers whose mask has bit c. This is NOT mtg_bubbles,
 * which counts what the compaction popped: that one keeps its meaning. */
typedef struct mtg_unitig_bubble_arrays {
    uint64_t *arm_off;       /* [bubbles + 1] */
    uint32_t *arm_unitig;    /* [arms] */
    uint8_t *arm_strand;     /* [arms] */
    uint32_t *arm_kmers;     /* [arms] */
    uint64_t *arm_abundance; /* [arms] */
    uint32_t *prefix;        /* [arms] */
    uint32_t *suffix;        /* [arms] */
    uint32_t *differences;   /* [arms] */
    uint32_t *carried;       /* [arms * n_colors], NULL without kmer_colors */
} mtg_unitig_bubble_arrays;
/* unitig_seqs / seq_offsets: the n_unitigs records of g's unitigs (ACGT), offsets from 0. unitig_kc: the abundance sum of every
 * unitig, or NULL. kmer_colors: NULL, or one 64-bit mask per k-mer in the order of the store's windows (record by record), with
 * n_colors in 1..64. Every array of *arrays is released with mtg_free. Fewer than 2^31 - 1 unitigs; an arm has fewer than 2^31 k-mers
 * whatever max_arm_kmers says. An empty graph, max_arm_kmers <= 1 and a graph without bubbles give 0 and arm_off = {0}. Returns the
 * bubbles. Aborts without a GPU: there is no CPU path. */
uint64_t mtg_unitig_bubbles(const mtg_graph *g, const char *unitig_seqs, const uint64_t *seq_offsets, uint64_t n_unitigs, uint64_t k,
                            uint64_t max_arm_kmers, const uint64_t *unitig_kc, const uint64_t *kmer_colors, uint32_t n_colors, int device_id,
                            mtg_unitig_bubble_arrays *arrays);
/* Of the last mtg_unitig_bubbles on this thread: {upload with the pack (host clock, ms), keys + group + number, allele kernel,
 * carrier kernel -- HIP events, ms --, download (host clock, ms), bubbles, arms, peak of the device arena's live bytes}. */
void mtg_last_unitig_bubbles_times(double out[8]);
/* Duplication bitvectors (implementation/mod.rs:668-702): one line per tig with `weight` characters per edge, '1' for an
 * original edge and '0' for a dummy edge (k-mers that repeat ones spelled elsewhere). */
uint64_t mtg_write_duplication_bitvector(const mtg_graph *g, uint64_t n_walks, const uint64_t *limits, const uint32_t *edges,
                                         char **text_out);
uint64_t mtg_write_tigs_duplication_bitvector_file(const mtg_graph *g, const mtg_walks *tigs, const char *path);

/* ---- synthetic input on the GPU (bench / test infrastructure; numpy twin: matchtigs_amd/synth.py g_csr) ---------------- */
/* G-csr(n_binodes mirror pairs + n_self_mirrors self-mirror nodes; n_unitigs candidate unitigs with uniform endpoints from the
 * counter-based splitmix64 streams of `seed`; a unitig whose directed edges would exceed max_degree at their from-nodes is
 * dropped; weight = 1 + #{j : x <= weight_thresholds[j]} with x the 53-bit uniform of stream 3 and the thresholds descending,
 * i.e. a clipped geometric distribution in integer form). Returns the built graph. Aborts without a GPU. */
mtg_graph *mtg_synth_g_csr(uint64_t n_binodes, uint64_t n_self_mirrors, uint64_t n_unitigs, uint64_t seed, uint64_t k,
                           const uint64_t *weight_thresholds, uint64_t n_thresholds, int max_degree, int device_id);

/* Whole path: algorithm 1, 3 or 5 (clib.rs ids). Mutates g. matchtigs_compute_tigs builds the configuration from
 * clib.rs:378-389's constants and calls this. */
mtg_walks *mtg_compute_tigs_cfg(mtg_graph *g, uint64_t tig_algorithm, const mtg_config *cfg);
/* The whole path into a caller's clib.rs output arrays (clib.rs:332-348: 2 E, 2 E and E entries for E original edges; layout as
 * mtg_flatten_clib / clib.rs:393-407): mtg_compute_tigs_cfg + mtg_flatten_clib in one call -- what matchtigs_compute_tigs runs.
 * With a finish on the GPU (the default) the tigs never exist as walks on the host: the threads that empty the download ring write
 * the flattened form straight into the caller's arrays. Mutates g like mtg_compute_tigs_cfg. Returns the number of tigs. */
uint64_t mtg_compute_tigs_clib(mtg_graph *g, uint64_t tig_algorithm, const mtg_config *cfg, int64_t *tigs_edge_out,
                               uint64_t *tigs_insert_out, uint64_t *tigs_out_limits);
/* The same with mtg_config_init(threads = 1, k) on GPU `device_id`. */
mtg_walks *mtg_compute_tigs(mtg_graph *g, uint64_t tig_algorithm, uint64_t k, int device_id);
/* Counters of the last mtg_compute_tigs_cfg(5) on this thread run with MTG_PERFORMANCE_DATA_COMPLETE (zeros otherwise). */
void mtg_last_performance_data(mtg_dijkstra_performance_data *out);

/* Phase timings (seconds) of the last mtg_compute_tigs on this thread:
 * [0] device build+upload, [1] classify, [2] sssp (all levels; with several GPUs + the gather), [3] download of the matched pairs
 * (0 when they stay in HBM for a finish on the same GPU), [4] claim replay,
 * [5] dummy insertion + Euleriser, [6] Euler decomposition, [7] cut. */
void mtg_last_phase_seconds(double out[8]);

#ifdef __cplusplus
}
#endif
#endif /* MTG_ENGINE_H */
