// engine_api.cpp -- extern "C" surface of libmatchtigs: include/mtg_engine.h and include/matchtigs.h.
//
// matchtigs_* are the drop-in replacements of /root/reference/src/clib.rs:87-410; mtg_* is the
// engine layer underneath (see the header for which reference lines each stage replaces).
#include <spawn.h>
#include <sys/mman.h>
#include <sys/wait.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <chrono>
#include <cstdarg>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/matchtigs.h"
#include "../../include/mtg_engine.h"
#include "../../include/mtg_policy.h"
#include "device.hpp"
#include "euler_lean.hpp"
#include "fastq_text.hpp"
#include "host_graph.hpp"
#include "hugebuf.hpp"
#include "parallel.hpp"

using namespace mtg;

extern char **environ;

struct mtg_graph { HostGraph g; };
struct mtg_device { Device *d; };
// The tigs of a finish on the GPU stay in HBM (`dev`) until somebody asks for them on the host: host() downloads them once. Counts
// come from `dev` without a copy; a clib.rs caller's tigs never get here (TigSink).
struct mtg_walks {
    mutable Walks w;
    mutable std::unique_ptr<ResidentTigs> dev;
    mutable std::mutex m;
    mtg_walks() = default;
    explicit mtg_walks(Walks &&walks, ResidentTigs *resident = nullptr) : w(std::move(walks)), dev(resident) {}
    const Walks &host() const {
        std::lock_guard<std::mutex> lock(m);
        if (dev) {
            dev->download(w);
            dev.reset();
        }
        return w;
    }
    Walks &host() { return const_cast<Walks &>(static_cast<const mtg_walks *>(this)->host()); }
    // (the device arrays, if the tigs are still on that GPU; valid until a call brings them to the host -- one thread per handle)
    const ResidentTigs *resident_on(int device_id) const {
        std::lock_guard<std::mutex> lock(m);
        return dev && dev->device == device_id ? dev.get() : nullptr;
    }
    uint64_t count() const {
        std::lock_guard<std::mutex> lock(m);
        return dev ? dev->n_tigs : w.limits.size();
    }
    uint64_t total_edges() const {
        std::lock_guard<std::mutex> lock(m);
        return dev ? dev->n_edges : w.edges.size();
    }
};
// The clib.rs handle is the same object as the engine graph.
struct MatchtigsData { mtg_graph graph; };

static thread_local double g_phase[8] = {0, 0, 0, 0, 0, 0, 0, 0};
static bool g_log_initialised = false;
static thread_local double g_last_euler_kernel_ms = 0;
static thread_local double g_last_gather_ms = 0;
static thread_local mtg_dijkstra_performance_data g_last_perf = {};
static thread_local double g_last_finish_times[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
// mtg_compute_tigs_clib: where a device finish on this thread delivers its tigs (the caller's clib.rs arrays) instead of a Walks object
static thread_local TigSink *g_clib_sink = nullptr;
static thread_local bool g_clib_sink_used = false;

static void check_config(const mtg_config *cfg, const char *who) {
    if (!cfg) MTG_DIE("%s: null configuration", who);
    // fields are only ever appended: an older caller's (shorter) struct is valid, a newer or a garbage one is not
    static_assert(sizeof(mtg_config) == MTG_CONFIG_MIN_SIZE, "a field was appended to mtg_config: read it only when cfg->struct_size covers it, and default it otherwise");
    if (cfg->struct_size < MTG_CONFIG_MIN_SIZE || cfg->struct_size > sizeof(mtg_config))
        MTG_DIE("%s: mtg_config.struct_size = %llu, this library understands %d to %zu bytes: fill the configuration with mtg_config_init, and "
                "build against an mtg_engine.h no newer than this library", who, (unsigned long long)cfg->struct_size, MTG_CONFIG_MIN_SIZE, sizeof(mtg_config));
    if (cfg->k < 1) MTG_DIE("%s: k must be >= 1", who);
    if (cfg->n_devices < 1 || cfg->n_devices > MTG_MAX_DEVICES) MTG_DIE("%s: n_devices = %d is out of range [1, %d]", who, cfg->n_devices, MTG_MAX_DEVICES);
    if (cfg->euler_mode != MTG_EULER_HOST_REFERENCE_ORDER && cfg->euler_mode != MTG_EULER_DEVICE) MTG_DIE("%s: unknown euler_mode %d", who, cfg->euler_mode);
    if (cfg->finish_stage != MTG_FINISH_AUTO && cfg->finish_stage != MTG_FINISH_HOST && cfg->finish_stage != MTG_FINISH_DEVICE)
        MTG_DIE("%s: unknown finish_stage %d", who, cfg->finish_stage);
    if (cfg->node_weight_array_type != MTG_NODE_WEIGHT_EPOCH_ARRAY && cfg->node_weight_array_type != MTG_NODE_WEIGHT_HASHBROWN_HASH_MAP)
        MTG_DIE("Unknown node weight array type: %d", cfg->node_weight_array_type);       // implementation/mod.rs:78
    if (cfg->heap_type != MTG_HEAP_STD_BINARY_HEAP) MTG_DIE("Unknown heap type: %d", cfg->heap_type);  // implementation/mod.rs:99
    if (cfg->performance_data_type != MTG_PERFORMANCE_DATA_NONE && cfg->performance_data_type != MTG_PERFORMANCE_DATA_COMPLETE)
        MTG_DIE("Unknown performance data type: %d", cfg->performance_data_type);          // implementation/mod.rs:123
}

static Walks euler_cycles_by_mode(const HostGraph &g, const mtg_config &cfg) {
    if (cfg.euler_mode == MTG_EULER_DEVICE) return device_euler_cycles(g, cfg.device_ids[0], &g_last_euler_kernel_ms);
    return euler_cycles(g);
}

static size_t tig_count(const mtg_walks *tigs) {  // (a device finish with a sink delivers no walks)
    return g_clib_sink && g_clib_sink_used ? (size_t)g_clib_sink->n_tigs : (size_t)tigs->count();
}
static double now_s() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
static void log_info(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
static void log_info(const char *fmt, ...) {
    if (!g_log_initialised) return;  // the reference logs nothing before matchtigs_initialise either
    va_list ap;
    va_start(ap, fmt);
    std::fprintf(stderr, "[INFO] ");
    std::vfprintf(stderr, fmt, ap);
    std::fprintf(stderr, "\n");
    va_end(ap);
}

// Giving a large graph back takes as long as unmapping its memory does (0.05 s for the edge arrays of the 2^27 graph, 1 s with the
// 23 GB of walk records a reference-order finish leaves in its arena): the device copy goes at once, the host memory on a thread
// of its own -- the caller (clib.rs:291 consumes the handle inside matchtigs_compute_tigs) has its result and does not wait for munmap.
template <typename T>
static void free_graph_object(T *obj, HostGraph &g) {
    if (!obj) return;
    if (g.edge_count() < (1u << 22)) {
        delete obj;
        return;
    }
    device_release_graph_cache(g);
    g.arena.unpin_all();  // (what is left for the thread makes no HIP call)
    std::thread([obj]() { delete obj; }).detach();
}

extern "C" {

const char *mtg_version(void) { return "matchtigs-amd 0.1 (gfx950; reference algbio/matchtigs 2.1.9)"; }
int mtg_device_count(void) { return device_count(); }
unsigned mtg_policies(void) { return MTG_POLICY_MASK; }

// ---- host graph ----
mtg_graph *mtg_graph_from_edges(uint64_t n_nodes, const uint32_t *mirror, uint64_t n_edges, const uint32_t *edge_from,
                                const uint32_t *edge_to, const uint64_t *edge_weight) {
    HostGraph *h = graph_from_edges(n_nodes, mirror, n_edges, edge_from, edge_to, edge_weight);
    mtg_graph *g = new mtg_graph{std::move(*h)};
    delete h;
    return g;
}
mtg_graph *mtg_graph_builder_new(uint64_t unitig_amount) {
    HostGraph *h = builder_new(unitig_amount);
    mtg_graph *g = new mtg_graph{std::move(*h)};
    delete h;
    return g;
}
void mtg_graph_builder_merge(mtg_graph *g, uint64_t ua, int sa, uint64_t ub, int sb) {
    if (!g) MTG_DIE("mtg_graph_builder_merge: null graph");
    builder_merge(&g->g, ua, sa != 0, ub, sb != 0);
}
void mtg_graph_builder_merge_links(mtg_graph *g, uint64_t n_links, const int64_t *links) {
    if (!g || (n_links && !links)) MTG_DIE("mtg_graph_builder_merge_links: null argument");
    for (uint64_t i = 0; i < n_links; i++) {
        if (links[4 * i] < 0 || links[4 * i + 2] < 0) MTG_DIE("mtg_graph_builder_merge_links: negative unitig id in row %llu", (unsigned long long)i);
        builder_merge(&g->g, (uint64_t)links[4 * i], links[4 * i + 1] != 0, (uint64_t)links[4 * i + 2], links[4 * i + 3] != 0);
    }
}
void mtg_graph_builder_build(mtg_graph *g, const uint64_t *unitig_weights) {
    if (!g) MTG_DIE("mtg_graph_builder_build: null graph");
    builder_build(&g->g, unitig_weights);
}
void mtg_graph_free(mtg_graph *g) {
    if (g) free_graph_object(g, g->g);
}
void mtg_graph_reset(mtg_graph *g) {
    if (!g || !g->g.built) MTG_DIE("mtg_graph_reset: graph is not built");
    g->g.reset_to_original();
}
uint64_t mtg_graph_node_count(const mtg_graph *g) { return g->g.node_count(); }
uint64_t mtg_graph_edge_count(const mtg_graph *g) { return g->g.edge_count(); }
// (the payload of an edge is kept per biedge, and only what is not arithmetic: host_graph.hpp)
static void export_payload(const HostGraph &h, uint64_t first, uint64_t n, uint64_t *edge_weight, uint64_t *edge_dummy_id, uint64_t *edge_unitig,
                           uint8_t *edge_forwards) {
    if (!edge_weight && !edge_dummy_id && !edge_unitig && !edge_forwards) return;
    parallel_ranges(n, [&](uint64_t lo, uint64_t hi) {
        for (uint64_t i = lo; i < hi; i++) {
            const uint64_t e = first + i;
            if (edge_weight) edge_weight[i] = h.weight(e);
            if (edge_dummy_id) edge_dummy_id[i] = h.dummy_id(e);
            if (edge_unitig) edge_unitig[i] = h.unitig(e);
            if (edge_forwards) edge_forwards[i] = h.forwards(e) ? 1 : 0;
        }
    });
}
void mtg_graph_export(const mtg_graph *g, uint32_t *mirror, uint32_t *edge_from, uint32_t *edge_to, uint64_t *edge_weight,
                      uint64_t *edge_dummy_id, uint64_t *edge_unitig, uint8_t *edge_forwards) {
    const HostGraph &h = g->g;
    const size_t V = h.node_count(), E = h.edge_count();
    if (mirror && V) std::memcpy(mirror, h.mirror.data(), V * 4);
    if (edge_from && E) std::memcpy(edge_from, h.e_from.data(), E * 4);
    if (edge_to && E) std::memcpy(edge_to, h.e_to.data(), E * 4);
    export_payload(h, 0, E, edge_weight, edge_dummy_id, edge_unitig, edge_forwards);
}

void mtg_graph_export_range(const mtg_graph *g, uint64_t first_edge, uint64_t n_edges, uint32_t *edge_from, uint32_t *edge_to,
                            uint64_t *edge_weight, uint64_t *edge_dummy_id, uint64_t *edge_unitig, uint8_t *edge_forwards) {
    const HostGraph &h = g->g;
    if (first_edge > h.edge_count() || n_edges > h.edge_count() - first_edge) MTG_DIE("mtg_graph_export_range: range exceeds the %llu edges", (unsigned long long)h.edge_count());
    if (!n_edges) return;
    const size_t o = first_edge, n = n_edges;
    if (edge_from) std::memcpy(edge_from, h.e_from.data() + o, n * 4);
    if (edge_to) std::memcpy(edge_to, h.e_to.data() + o, n * 4);
    export_payload(h, o, n, edge_weight, edge_dummy_id, edge_unitig, edge_forwards);
}
uint64_t mtg_graph_original_edge_count(const mtg_graph *g) { return g->g.n_original_edges; }

// ---- device stage ----
mtg_device *mtg_device_create(const mtg_graph *g, uint64_t k, int device_id) {
    if (!g || !g->g.built) MTG_DIE("mtg_device_create: graph is not built");
    // (a unitig of weight 0 aborts inside device_create, in the pass that clamps the weights: the bounded search and its lower
    // bounds need weights >= 1 -- the reference computes weight = len + 1 - k >= 1, bin.rs:369-376)
    return new mtg_device{device_create(g->g, k, device_id)};
}
mtg_device *mtg_device_create_opts(const mtg_graph *g, uint64_t k, int device_id, int flags) {
    if (!g || !g->g.built) MTG_DIE("mtg_device_create_opts: graph is not built");
    if (flags & ~(MTG_DEVICE_NO_LOWER_BOUNDS | MTG_DEVICE_RESERVE_WORK)) MTG_DIE("mtg_device_create_opts: unknown flags %d", flags);
    mtg_device *d = new mtg_device{device_create(g->g, k, device_id, !(flags & MTG_DEVICE_NO_LOWER_BOUNDS))};
    if (flags & MTG_DEVICE_RESERVE_WORK) device_reserve_step_work(d->d);
    const int used[1] = {device_id};
    device_drop_foreign_reservation(used, 1);  // (a constructor's provisional chunk on another GPU goes back)
    return d;
}
void mtg_device_build_lower_bounds(mtg_device *d, void *stream) {
    if (!d) MTG_DIE("mtg_device_build_lower_bounds: null device");
    device_build_lower_bounds(d->d, stream);
}
double mtg_device_lower_bounds_ms(const mtg_device *d) { return d ? device_lower_bounds_ms(d->d) : 0.0; }
void mtg_device_free(mtg_device *d) {
    if (!d) return;
    device_free(d->d);
    delete d;
}
uint64_t mtg_device_graph_bytes(const mtg_device *d) { return device_graph_bytes(d->d); }
uint64_t mtg_classify(mtg_device *d, void *stream) { return device_classify(d->d, stream); }
void mtg_classify_download(mtg_device *d, void *stream, uint32_t *out_nodes, int32_t *multiplicity, uint8_t *is_in_node) {
    device_classify_download(d->d, stream, out_nodes, multiplicity, is_in_node);
}
const uint32_t *mtg_classify_d_out_nodes(const mtg_device *d) { return device_d_out_nodes(d->d); }
int mtg_sssp_candidates(mtg_device *d, void *stream, uint64_t src_begin, uint64_t src_end, uint64_t *d_pool,
                        uint64_t pool_capacity, uint64_t *d_cand_start, uint32_t *d_cand_count, uint64_t *pool_needed) {
    return device_sssp(d->d, stream, src_begin, src_end, d_pool, pool_capacity, d_cand_start, d_cand_count, pool_needed);
}
double mtg_last_sssp_kernel_ms(const mtg_device *d) { return device_last_kernel_ms(d->d); }
int mtg_last_sssp_levels(const mtg_device *d, double *ms_out, uint64_t *sources_out, int capacity) {
    return device_last_levels(d->d, ms_out, sources_out, capacity);
}
const char *mtg_last_sssp_level_name(const mtg_device *d, int level) { return device_last_level_name(d->d, level); }
void mtg_sssp_count(mtg_device *d, void *stream, uint64_t src_begin, uint64_t src_end, mtg_sssp_stats *stats) {
    device_sssp_count(d->d, stream, src_begin, src_end, stats);
}
void mtg_sssp_count_visited(mtg_device *d, void *stream, uint64_t src_begin, uint64_t src_end, mtg_sssp_stats *stats) {
    device_sssp_count_visited(d->d, stream, src_begin, src_end, stats);
}
int mtg_sssp_prunes(const mtg_device *d) { return device_prunes(d->d) ? 1 : 0; }
uint64_t mtg_last_sssp_searched_sources(const mtg_device *d) { return device_last_active_sources(d->d); }
int mtg_set_sssp_plan(mtg_device *d, int plan) { return device_set_plan(d->d, plan); }
uint64_t mtg_replay_claims_device(mtg_device *d, void *stream, uint64_t n_sources, const uint64_t *d_cand_start,
                                  const uint32_t *d_cand_count, const uint64_t *d_pool, mtg_pair **pairs_out) {
    if (!d || !pairs_out) MTG_DIE("mtg_replay_claims_device: null argument");
    return device_replay(d->d, stream, n_sources, d_cand_start, d_cand_count, d_pool, pairs_out, nullptr);
}
void mtg_last_replay_ms(const mtg_device *d, double out[2]) { device_last_replay_ms(d->d, out); }
void mtg_set_replay_tuning(mtg_device *d, uint64_t windows, int block, int grid, int role_mod, int plain_barrier) {
    if (!d) MTG_DIE("mtg_set_replay_tuning: null device");
    device_set_replay_tuning(d->d, windows, block, grid, role_mod, plain_barrier);
}
uint64_t mtg_replay_claims_resident(mtg_device *d, void *stream, uint64_t n_sources, const uint64_t *d_cand_start,
                                    const uint32_t *d_cand_count, const uint64_t *d_pool) {
    if (!d) MTG_DIE("mtg_replay_claims_resident: null argument");
    return device_replay(d->d, stream, n_sources, d_cand_start, d_cand_count, d_pool, nullptr, nullptr);
}
const mtg_pair *mtg_resident_pairs(const mtg_device *d, uint64_t *n_pairs_out) {
    if (!d) MTG_DIE("mtg_resident_pairs: null argument");
    return device_resident_pairs(d->d, n_pairs_out);
}
uint64_t mtg_download_resident_pairs(mtg_device *d, mtg_pair **pairs_out) {
    if (!d || !pairs_out) MTG_DIE("mtg_download_resident_pairs: null argument");
    return device_download_pairs(d->d, pairs_out);
}
int mtg_last_replay_rounds(const mtg_device *d) { return device_last_replay_rounds(d->d); }
uint64_t mtg_last_replay_visits(const mtg_device *d) { return device_last_replay_visits(d->d); }
uint64_t mtg_compute_pairs(mtg_device *const *devices, int n_devices, mtg_pair **pairs_out) {
    if (!devices || n_devices < 1 || n_devices > MTG_MAX_DEVICES || !pairs_out) MTG_DIE("mtg_compute_pairs: bad argument");
    std::vector<Device *> dv;
    for (int i = 0; i < n_devices; i++) {
        if (!devices[i]) MTG_DIE("mtg_compute_pairs: null device %d", i);
        dv.push_back(devices[i]->d);
    }
    return device_pairs_multi(dv.data(), n_devices, pairs_out, nullptr, &g_last_gather_ms);
}
double mtg_last_gather_ms(void) { return g_last_gather_ms; }
void mtg_partition_sources(mtg_device *d, int parts, uint64_t *cuts_out) {
    if (!d || parts < 1 || !cuts_out) MTG_DIE("mtg_partition_sources: bad argument");
    const std::vector<uint64_t> c = device_partition_sources(d->d, nullptr, parts);
    for (int i = 0; i <= parts; i++) cuts_out[i] = c[(size_t)i];
}

// ---- host stages ----
uint64_t mtg_replay_claims(const mtg_graph *g, uint64_t n_sources, const uint32_t *out_nodes, const int32_t *multiplicity,
                           const uint8_t *is_in_node, const uint64_t *cand_start, const uint32_t *cand_count,
                           const uint64_t *pool, mtg_pair **pairs_out) {
    std::vector<Pair> p = replay_claims(g->g, n_sources, out_nodes, multiplicity, is_in_node, cand_start, cand_count, pool);
    static_assert(sizeof(Pair) == sizeof(mtg_pair), "pair layout");
    mtg_pair *out = (mtg_pair *)std::malloc(std::max<size_t>(p.size(), 1) * sizeof(mtg_pair));
    if (!out) MTG_DIE("out of memory");
    if (!p.empty()) std::memcpy(out, p.data(), p.size() * sizeof(mtg_pair));
    *pairs_out = out;
    return p.size();
}
void mtg_free(void *p) { std::free(p); }

uint64_t mtg_insert_pair_edges(mtg_graph *g, const mtg_pair *pairs, uint64_t n_pairs) {
    return insert_pair_edges(g->g, reinterpret_cast<const Pair *>(pairs), n_pairs);
}
uint64_t mtg_make_eulerian(mtg_graph *g, uint64_t dummy_edge_id, uint64_t k) { return make_eulerian(g->g, dummy_edge_id, k); }
mtg_walks *mtg_euler_cycles(const mtg_graph *g) { return new mtg_walks{euler_cycles(g->g)}; }
mtg_walks *mtg_euler_cycles_records(const mtg_graph *g, int record_format) {
    const HostGraph &h = g->g;
    if (record_format == 0) return new mtg_walks{euler_cycles(h)};
    if (record_format < 1 || record_format > 3) MTG_DIE("mtg_euler_cycles_records: unknown record format %d", record_format);
    h.ensure_linked();
    const uint64_t V = h.node_count(), E = h.edge_count();
    std::vector<LeanNode> lean(V);
    std::vector<uint32_t> ext_eid, ext_to;
    for (uint64_t n = 0; n < V; n++) {  // what lean_build_kernel writes (finish_device.hip): own adjacency, newest edge first
        LeanNode &r = lean[n];
        if (h.out_deg[n] > 65535) MTG_DIE("mtg_euler_cycles_records: out-degree beyond 65535");
        r.deg = (uint16_t)h.out_deg[n];
        r.pos = 0;
        r.ext_begin = (uint32_t)ext_eid.size();
        for (int i = 0; i < 3; i++) r.eid[i] = r.to[i] = NONE;
        uint32_t i = 0;
        for (uint32_t e = h.head_out[n]; e != NONE; e = h.e_next_out[e], i++) {
            if (i < 3) { r.eid[i] = e; r.to[i] = h.e_to[e]; }
            else { ext_eid.push_back(e); ext_to.push_back(h.e_to[e]); }
        }
    }
    if (record_format == 1)
        return new mtg_walks{euler_cycles_lean(lean.data(), V, ext_eid.data(), ext_to.data(), h.e_from.data(), h.e_to.data(), E, &h.arena)};
    if (record_format == 3) {
        HugeBuf<EulerNode2> mid(V, &h.arena);
        return new mtg_walks{euler_cycles_from_lean_mid(lean.data(), mid.p, V, ext_eid.data(), ext_to.data(), h.e_from.data(), h.e_to.data(), E, &h.arena)};
    }
    HugeBuf<EulerNode3> wide(V, &h.arena);
    return new mtg_walks{euler_cycles_from_lean(lean.data(), wide.p, V, ext_eid.data(), ext_to.data(), h.e_from.data(), h.e_to.data(), E, &h.arena)};
}
mtg_walks *mtg_euler_cycles_device(const mtg_graph *g, int device_id) {
    return new mtg_walks{device_euler_cycles(g->g, device_id, &g_last_euler_kernel_ms)};
}
double mtg_last_euler_kernel_ms(void) { return g_last_euler_kernel_ms; }
void mtg_set_euler_device_tuning(int splitter_bitmap) { device_euler_force_bitmap(splitter_bitmap); }
mtg_walks *mtg_cut_cycles(const mtg_graph *g, const mtg_walks *cycles, uint64_t k) {
    return new mtg_walks{cut_cycles(g->g, cycles->host(), k)};
}

// The device finish takes a graph that holds only its original edges and matched pairs shorter than k (what the claim loop
// produces); anything else (a graph Eulerised before, pairs from elsewhere) goes through the generic host stages.
static bool use_device_finish(const HostGraph &g, const mtg_pair *pairs, uint64_t n_pairs, const mtg_config &cfg) {
    if (cfg.finish_stage == MTG_FINISH_HOST) return false;
    const bool forced = cfg.finish_stage == MTG_FINISH_DEVICE;
    if (device_count() <= cfg.device_ids[0]) {
        if (forced) MTG_DIE("finish_stage = MTG_FINISH_DEVICE, but no MI355X/HIP device %d is visible", cfg.device_ids[0]);
        return false;
    }
    bool ok = g.edge_count() == g.n_original_edges && g.first_breaking_edge == UINT64_MAX && cfg.k <= 0xFFFFFFFFull;
    for (uint64_t i = 0; i < n_pairs && ok; i++) ok = pairs[i].distance < cfg.k && pairs[i].out_node < g.node_count() && pairs[i].in_node < g.node_count();
    if (!ok && forced) MTG_DIE("finish_stage = MTG_FINISH_DEVICE needs a graph without dummy edges and matched pairs shorter than k");
    return ok;
}
static mtg_walks *finish_on_device(HostGraph &g, const mtg_pair *pairs, uint64_t n_pairs, const mtg_config &cfg, const mtg_pair *d_pairs_resident = nullptr) {
    log_info("Making graph Eulerian by adding breaking dummy edges");
    log_info("Finding Eulerian bicycle");
    double *t = g_last_finish_times;
    if (g_clib_sink) g_clib_sink_used = true;
    ResidentTigs *resident = nullptr;
    Walks host_walks = device_finish(g, reinterpret_cast<const Pair *>(pairs), n_pairs, cfg.k, cfg.device_ids[0], cfg.euler_mode, t, d_pairs_resident, g_clib_sink,
                                     g_clib_sink ? nullptr : &resident);
    mtg_walks *tigs = new mtg_walks(std::move(host_walks), resident);
    g_phase[5] = t[0] + t[1];
    g_phase[6] = t[2];
    g_phase[7] = t[3];
    g_last_euler_kernel_ms = t[4];
    return tigs;
}

static mtg_walks *eulerise_and_cut(HostGraph &g, uint64_t dummy_edge_id, const mtg_config &cfg) {
    const uint64_t k = cfg.k;
    double t0 = now_s();
    log_info("Making graph Eulerian by adding breaking dummy edges");
    make_eulerian(g, dummy_edge_id, k);
    if (!is_eulerian(g)) MTG_DIE("Failed to make the graph Eulerian. (greedytigs/mod.rs:714)");
    double t1 = now_s();
    g_phase[5] += t1 - t0;
    log_info("Finding Eulerian bicycle");
    Walks cycles = euler_cycles_by_mode(g, cfg);
    double t2 = now_s();
    g_phase[6] = t2 - t1;
    log_info("Found %zu Eulerian bicycles", cycles.limits.size());
    mtg_walks *tigs = new mtg_walks{cut_cycles(g, cycles, k)};
    g_phase[7] = now_s() - t2;
    return tigs;
}

void mtg_config_init(mtg_config *cfg, uint64_t threads, uint64_t k) {  // GreedytigAlgorithmConfiguration::new, greedytigs/mod.rs:62-72
    if (!cfg) MTG_DIE("mtg_config_init: null configuration");
    std::memset(cfg, 0, sizeof *cfg);
    cfg->struct_size = sizeof *cfg;
    cfg->threads = threads;
    cfg->k = k;
    cfg->staged_parallelism_divisor = 0.0;
    cfg->resource_limit_factor = 0;
    cfg->node_weight_array_type = MTG_NODE_WEIGHT_HASHBROWN_HASH_MAP;
    cfg->heap_type = MTG_HEAP_STD_BINARY_HEAP;
    cfg->performance_data_type = MTG_PERFORMANCE_DATA_NONE;
    cfg->euler_mode = MTG_EULER_HOST_REFERENCE_ORDER;
    cfg->finish_stage = MTG_FINISH_AUTO;
    cfg->n_devices = 1;
    cfg->device_ids[0] = 0;
}

mtg_walks *mtg_finish_greedytigs_cfg(mtg_graph *g, const mtg_pair *pairs, uint64_t n_pairs, const mtg_config *cfg) {
    check_config(cfg, "mtg_finish_greedytigs_cfg");
    if (!g || !g->g.built) MTG_DIE("mtg_finish_greedytigs_cfg: graph is not built");
    if (n_pairs && !pairs) MTG_DIE("mtg_finish_greedytigs_cfg: null pairs");
    if (use_device_finish(g->g, pairs, n_pairs, *cfg)) {
        mtg_walks *tigs = finish_on_device(g->g, pairs, n_pairs, *cfg);
        log_info("Found %zu greedytigs", tig_count(tigs));
        return tigs;
    }
    double t0 = now_s();
    const uint64_t dummy_edge_id = insert_pair_edges(g->g, reinterpret_cast<const Pair *>(pairs), n_pairs);
    g_phase[5] = now_s() - t0;
    mtg_walks *tigs = eulerise_and_cut(g->g, dummy_edge_id, *cfg);
    log_info("Found %zu greedytigs", tig_count(tigs));
    return tigs;
}
mtg_walks *mtg_finish_device(mtg_graph *g, const mtg_pair *pairs, uint64_t n_pairs, const mtg_config *cfg) {
    check_config(cfg, "mtg_finish_device");
    if (!g || !g->g.built) MTG_DIE("mtg_finish_device: graph is not built");
    if (n_pairs && !pairs) MTG_DIE("mtg_finish_device: null pairs");
    mtg_config forced = *cfg;
    forced.finish_stage = MTG_FINISH_DEVICE;
    (void)use_device_finish(g->g, pairs, n_pairs, forced);
    return finish_on_device(g->g, pairs, n_pairs, forced);
}
mtg_walks *mtg_finish_greedytigs_resident(mtg_graph *g, mtg_device *d, const mtg_config *cfg) {
    check_config(cfg, "mtg_finish_greedytigs_resident");
    if (!g || !g->g.built || !d) MTG_DIE("mtg_finish_greedytigs_resident: graph is not built / null device");
    // (the resident pairs index the graph d was built from, and their distances are below d's k: the host path checks every pair
    // it is handed, here the identity of the graph stands for that)
    if (!device_matches(d->d, g->g, cfg->k))
        MTG_DIE("mtg_finish_greedytigs_resident: the device copy was built from another graph (node / edge counts differ) or for another k than cfg->k = %llu",
                (unsigned long long)cfg->k);
    uint64_t n_pairs = 0;
    const mtg_pair *d_pairs = device_resident_pairs(d->d, &n_pairs);
    if (use_device_finish(g->g, nullptr, 0, *cfg) && device_id_of(d->d) == cfg->device_ids[0]) {
        mtg_walks *tigs = finish_on_device(g->g, nullptr, n_pairs, *cfg, d_pairs);
        log_info("Found %zu greedytigs", tig_count(tigs));
        return tigs;
    }
    // host finish, or a finish on another GPU: through the host, like mtg_finish_greedytigs_cfg
    mtg_pair *pairs = nullptr;
    n_pairs = device_download_pairs(d->d, &pairs);
    mtg_walks *tigs = mtg_finish_greedytigs_cfg(g, pairs, n_pairs, cfg);
    std::free(pairs);
    return tigs;
}
void mtg_release_device_memory(int device_id) { device_release_memory(device_id); }
void mtg_set_default_device(int device_id) {
    if (device_id < 0 || device_id >= 64) MTG_DIE("mtg_set_default_device: device id %d out of range", device_id);
    device_set_default(device_id);
}
void mtg_set_reserve_ahead(int on) { device_set_reserve_ahead(on); }
void mtg_set_finish_tuning(int records, int flags, int64_t record_delay_us) {
    if (records < 0 || records > 3) MTG_DIE("mtg_set_finish_tuning: unknown record format %d", records);
    device_set_finish_tuning(records, flags, (long)record_delay_us);
}
uint64_t mtg_device_memory_held(int device_id) { return device_memory_held(device_id); }
void mtg_device_arena_stats(int device_id, uint64_t out[4], int reset_peak) {
    if (device_id < 0 || device_id >= 64) MTG_DIE("mtg_device_arena_stats: device id %d out of range", device_id);
    device_arena_stats(device_id, out);
    if (reset_peak) device_arena_reset_peak(device_id);
}
void mtg_graph_release_device_cache(mtg_graph *g) {
    if (g) device_release_graph_cache(g->g);
}
void mtg_last_finish_device_times(double out[6]) {
    for (int i = 0; i < 6; i++) out[i] = g_last_finish_times[i];
}
void mtg_last_finish_device_stage_ms(double out[6]) {
    const double *t = g_last_finish_times;
    out[0] = t[6]; out[1] = t[7]; out[2] = t[4]; out[3] = t[8]; out[4] = t[9]; out[5] = t[10];
}
mtg_graph *mtg_synth_g_csr(uint64_t n_binodes, uint64_t n_self_mirrors, uint64_t n_unitigs, uint64_t seed, uint64_t k,
                           const uint64_t *weight_thresholds, uint64_t n_thresholds, int max_degree, int device_id) {
    if (n_thresholds && !weight_thresholds) MTG_DIE("mtg_synth_g_csr: null thresholds");
    HostGraph *h = device_synth_g_csr(n_binodes, n_self_mirrors, n_unitigs, seed, k, weight_thresholds, n_thresholds, max_degree, device_id);
    mtg_graph *g = new mtg_graph{std::move(*h)};
    delete h;
    return g;
}
mtg_walks *mtg_finish_greedytigs(mtg_graph *g, const mtg_pair *pairs, uint64_t n_pairs, uint64_t k) {
    mtg_config cfg;
    mtg_config_init(&cfg, 1, k);
    return mtg_finish_greedytigs_cfg(g, pairs, n_pairs, &cfg);
}
mtg_walks *mtg_compute_eulertigs_cfg(mtg_graph *g, const mtg_config *cfg) {
    check_config(cfg, "mtg_compute_eulertigs_cfg");
    if (!g || !g->g.built) MTG_DIE("mtg_compute_eulertigs_cfg: graph is not built");
    g_phase[5] = 0;
    mtg_walks *tigs = use_device_finish(g->g, nullptr, 0, *cfg) ? finish_on_device(g->g, nullptr, 0, *cfg)
                                                                : eulerise_and_cut(g->g, 0, *cfg);  // eulertigs/mod.rs:101-102
    log_info("Found %zu eulertigs", tig_count(tigs));
    return tigs;
}
mtg_walks *mtg_compute_eulertigs(mtg_graph *g, uint64_t k) {
    mtg_config cfg;
    mtg_config_init(&cfg, 1, k);
    return mtg_compute_eulertigs_cfg(g, &cfg);
}

uint64_t mtg_walks_count(const mtg_walks *w) { return w->count(); }
uint64_t mtg_walks_total_edges(const mtg_walks *w) { return w->total_edges(); }
void mtg_walks_export(const mtg_walks *w, uint64_t *limits, uint32_t *edges) {
    const Walks &h = w->host();
    if (limits && !h.limits.empty()) std::memcpy(limits, h.limits.data(), h.limits.size() * 8);
    if (edges && !h.edges.empty()) std::memcpy(edges, h.edges.data(), h.edges.size() * 4);
}
void mtg_walks_data(const mtg_walks *w, const uint64_t **limits, const uint32_t **edges) {
    const Walks &h = w->host();
    if (limits) *limits = h.limits.data();
    if (edges) *edges = h.edges.data();
}
void mtg_walks_free(mtg_walks *w) { delete w; }
mtg_walks *mtg_walks_from_arrays(uint64_t n_walks, const uint64_t *limits, const uint32_t *edges) {
    if (n_walks && (!limits || !edges)) MTG_DIE("mtg_walks_from_arrays: null argument");
    mtg_walks *w = new mtg_walks();
    uint64_t prev = 0;
    for (uint64_t i = 0; i < n_walks; i++) {
        if (limits[i] < prev) MTG_DIE("mtg_walks_from_arrays: limits must be non-decreasing");
        prev = limits[i];
    }
    w->w.limits.assign(limits, limits + n_walks);
    w->w.edges.assign(edges, edges + prev);
    return w;
}

uint64_t mtg_flatten_clib(const mtg_graph *g, const mtg_walks *tigs, int64_t *tigs_edge_out, uint64_t *tigs_insert_out,
                          uint64_t *tigs_out_limits) {
    return flatten_clib(g->g, tigs->host(), tigs_edge_out, tigs_insert_out, tigs_out_limits);
}

uint64_t mtg_write_walks_fasta(const mtg_graph *g, uint64_t n_walks, const uint64_t *limits, const uint32_t *edges, uint64_t k,
                               const char *unitig_seqs, const uint64_t *seq_offsets, char **fasta_out) {
    if (!g || !fasta_out || (n_walks && (!limits || !edges)) || !unitig_seqs || !seq_offsets)
        MTG_DIE("mtg_write_walks_fasta: null argument");
    return write_walks_fasta(g->g, n_walks, limits, edges, k, unitig_seqs, seq_offsets, fasta_out);
}

uint64_t mtg_write_walks_gfa(const mtg_graph *g, uint64_t n_walks, const uint64_t *limits, const uint32_t *edges, uint64_t k,
                             const char *unitig_seqs, const uint64_t *seq_offsets, const char *header, char **gfa_out) {
    if (!g || !gfa_out || (n_walks && (!limits || !edges)) || !unitig_seqs || !seq_offsets)
        MTG_DIE("mtg_write_walks_gfa: null argument");
    return write_walks_text(g->g, n_walks, limits, edges, k, unitig_seqs, seq_offsets, true, header, gfa_out);
}

// f-1 on the device: the same text from spell_device.hip (2-bit packed store, output-centric kernel)
static thread_local double g_last_spell_kernel_ms = 0;
static thread_local uint64_t g_last_spell_bytes = 0;
uint64_t mtg_write_walks_text_device(const mtg_graph *g, uint64_t n_walks, const uint64_t *limits, const uint32_t *edges, uint64_t k,
                                     const char *unitig_seqs, const uint64_t *seq_offsets, int gfa, const char *gfa_header, int device_id,
                                     char **text_out) {
    if (!g || !text_out || (n_walks && (!limits || !edges)) || !unitig_seqs || !seq_offsets)
        MTG_DIE("mtg_write_walks_text_device: null argument");
    return device_write_walks_text(g->g, n_walks, limits, edges, k, unitig_seqs, seq_offsets, gfa != 0, gfa_header, device_id, text_out,
                                   &g_last_spell_kernel_ms, &g_last_spell_bytes);
}
double mtg_last_spell_kernel_ms(void) { return g_last_spell_kernel_ms; }
uint64_t mtg_last_spell_bytes(void) { return g_last_spell_bytes; }

// ---- the unitig graph with its links (unitig_links_device.hip) ----
static thread_local UnitigGraphTimes g_last_unitig_graph;
uint64_t mtg_unitig_links(const mtg_graph *g, int device_id, uint64_t **link_off, uint32_t **link_to) {
    if (!g || !link_off || !link_to) MTG_DIE("mtg_unitig_links: null argument");
    return device_unitig_links(g->g, device_id, link_off, link_to, &g_last_unitig_graph);
}
uint64_t mtg_write_unitig_graph_text(const mtg_graph *g, const char *unitig_seqs, const uint64_t *seq_offsets, uint64_t n_unitigs, uint64_t k,
                                     const uint64_t *unitig_kc, int gfa, int device_id, char **text_out) {
    if (!g || !text_out || !seq_offsets || (n_unitigs && !unitig_seqs)) MTG_DIE("mtg_write_unitig_graph_text: null argument");
    return device_write_unitig_graph_text(g->g, unitig_seqs, seq_offsets, n_unitigs, k, unitig_kc, gfa != 0, device_id, text_out,
                                          &g_last_unitig_graph);
}
uint64_t mtg_write_unitig_graph_file(const mtg_graph *g, const char *unitig_seqs, const uint64_t *seq_offsets, uint64_t n_unitigs, uint64_t k,
                                     const uint64_t *unitig_kc, int gfa, int device_id, const char *path, int compression_level) {
    if (!path) MTG_DIE("mtg_write_unitig_graph_file: null argument");
    char *buf = nullptr;
    const uint64_t n = mtg_write_unitig_graph_text(g, unitig_seqs, seq_offsets, n_unitigs, k, unitig_kc, gfa, device_id, &buf);
    write_file(path, buf, n, compression_level);
    std::free(buf);
    return n;
}
void mtg_last_unitig_graph_times(double out[9]) {
    const UnitigGraphTimes &t = g_last_unitig_graph;
    out[0] = t.upload_ms; out[1] = t.link_ms; out[2] = t.text_prepare_ms; out[3] = t.text_ms; out[4] = t.download_ms;
    out[5] = (double)t.links; out[6] = (double)t.bytes; out[7] = (double)t.text_min_bytes; out[8] = (double)t.peak_arena_bytes;
}

// ---- the connected components of the unitig graph (unitig_components_device.hip) ----
static thread_local UnitigComponentsTimes g_last_unitig_components;
static std::atomic<int> g_unitig_components_aggregation{1};
void mtg_set_unitig_components_aggregation(int on) { g_unitig_components_aggregation.store(on ? 1 : 0); }
uint64_t mtg_unitig_components(const mtg_graph *g, const uint64_t *unitig_kmers, const uint64_t *unitig_kc, int device_id,
                               uint32_t **component_of, mtg_component_arrays *components) {
    if (!g || !component_of || !components) MTG_DIE("mtg_unitig_components: null argument");
    UnitigComponentArrays a;
    const uint64_t n = device_unitig_components(g->g, unitig_kmers, unitig_kc, device_id, g_unitig_components_aggregation.load() != 0, component_of,
                                                &a, &g_last_unitig_components);
    components->first_unitig = a.first_unitig; components->unitigs = a.unitigs; components->kmers = a.kmers;
    components->abundance = a.abundance; components->links = a.links; components->dead_ends = a.dead_ends;
    components->irregular = a.irregular;
    return n;
}
void mtg_last_unitig_components_times(double out[10]) {
    const UnitigComponentsTimes &t = g_last_unitig_components;
    out[0] = t.upload_ms; out[1] = t.label_ms; out[2] = t.stats_ms; out[3] = t.download_ms;
    out[4] = (double)t.components; out[5] = (double)t.unitigs; out[6] = (double)t.peak_arena_bytes;
    out[7] = t.rep_ms; out[8] = t.union_ms; out[9] = t.flatten_ms;
}

// ---- the bubbles of the unitig graph as variant calls (unitig_bubbles_device.hip) ----
static thread_local UnitigBubblesTimes g_last_unitig_bubbles;
uint64_t mtg_unitig_bubbles(const mtg_graph *g, const char *unitig_seqs, const uint64_t *seq_offsets, uint64_t n_unitigs, uint64_t k,
                            uint64_t max_arm_kmers, const uint64_t *unitig_kc, const uint64_t *kmer_colors, uint32_t n_colors, int device_id,
                            mtg_unitig_bubble_arrays *arrays) {
    if (!g || !arrays || !seq_offsets || (n_unitigs && !unitig_seqs)) MTG_DIE("mtg_unitig_bubbles: null argument");
    UnitigBubbleArrays a;
    const uint64_t n = device_unitig_bubbles(g->g, unitig_seqs, seq_offsets, n_unitigs, k, max_arm_kmers, unitig_kc, kmer_colors, n_colors, device_id,
                                             &a, &g_last_unitig_bubbles);
    arrays->arm_off = a.arm_off; arrays->arm_unitig = a.arm_unitig; arrays->arm_strand = a.arm_strand; arrays->arm_kmers = a.arm_kmers;
    arrays->arm_abundance = a.arm_abundance; arrays->prefix = a.prefix; arrays->suffix = a.suffix; arrays->differences = a.differences;
    arrays->carried = a.carried;
    return n;
}
void mtg_last_unitig_bubbles_times(double out[8]) {
    const UnitigBubblesTimes &t = g_last_unitig_bubbles;
    out[0] = t.upload_ms; out[1] = t.group_ms; out[2] = t.allele_ms; out[3] = t.carrier_ms; out[4] = t.download_ms;
    out[5] = (double)t.bubbles; out[6] = (double)t.arms; out[7] = (double)t.peak_arena_bytes;
}

uint64_t mtg_write_duplication_bitvector(const mtg_graph *g, uint64_t n_walks, const uint64_t *limits, const uint32_t *edges,
                                         char **text_out) {
    if (!g || !text_out || (n_walks && (!limits || !edges))) MTG_DIE("mtg_write_duplication_bitvector: null argument");
    return write_duplication_bitvector(g->g, n_walks, limits, edges, text_out);
}
uint64_t mtg_write_tigs_duplication_bitvector_file(const mtg_graph *g, const mtg_walks *tigs, const char *path) {
    if (!g || !tigs || !path) MTG_DIE("mtg_write_tigs_duplication_bitvector_file: null argument");
    char *buf = nullptr;
    const uint64_t n = write_duplication_bitvector(g->g, tigs->host().limits.size(), tigs->host().limits.data(), tigs->host().edges.data(), &buf);
    write_file(path, buf, n, 0);  // the reference writes this file uncompressed (implementation/mod.rs:665)
    std::free(buf);
    return n;
}

// ---- f-2: BCALM2 input route + FASTA file output ----
struct mtg_unitigs { UnitigStore *s; };

mtg_graph *mtg_read_bcalm2(const char *path, uint64_t k, mtg_unitigs **unitigs_out) {
    if (!unitigs_out) MTG_DIE("mtg_read_bcalm2: null argument");
    UnitigStore *st = nullptr;
    HostGraph *h = read_bcalm2(path, k, &st);
    mtg_graph *g = new mtg_graph{std::move(*h)};
    delete h;
    *unitigs_out = new mtg_unitigs{st};
    return g;
}
// ---- the plain unitig FASTA route: (k-1)-mer join on the GPU (fasta_in_device.hip) ----
static thread_local FastaJoinTimes g_last_fasta_in;
mtg_graph *mtg_read_fasta(const char *path, uint64_t k, int device_id, mtg_unitigs **unitigs_out) {
    if (!unitigs_out) MTG_DIE("mtg_read_fasta: null argument");
    UnitigStore *st = nullptr;
    HostGraph *h = read_fasta(path, k, device_id, &st, &g_last_fasta_in);
    mtg_graph *g = new mtg_graph{std::move(*h)};
    delete h;
    *unitigs_out = new mtg_unitigs{st};
    return g;
}
mtg_graph *mtg_graph_from_sequences(const char *data, const uint64_t *offsets, uint64_t n, uint64_t k, int device_id) {
    HostGraph *h = device_graph_from_sequences(data, offsets, n, k, device_id, &g_last_fasta_in);
    mtg_graph *g = new mtg_graph{std::move(*h)};
    delete h;
    return g;
}
void mtg_last_fasta_in_times(double out[6]) {
    const FastaJoinTimes &t = g_last_fasta_in;
    out[0] = t.parse_ms; out[1] = t.upload_ms; out[2] = t.kernel_ms; out[3] = t.download_ms; out[4] = t.build_ms; out[5] = (double)t.bytes;
}
// ---- k-mer set comparison on the GPU (kmer_compare_device.hip) ----
static thread_local KmerCompareTimes g_last_kmer_compare;
void mtg_compare_kmer_sets(const char *seq_a, const uint64_t *off_a, uint64_t n_a, const char *seq_b, const uint64_t *off_b, uint64_t n_b,
                           uint64_t k, int device_id, mtg_kmer_comparison *out) {
    device_compare_kmer_sets(seq_a, off_a, n_a, seq_b, off_b, n_b, k, device_id, out, &g_last_kmer_compare);
}
void mtg_compare_kmer_sets_stores(const mtg_unitigs *store_a, const mtg_unitigs *store_b, uint64_t k, int device_id, mtg_kmer_comparison *out) {
    if (!store_a || !store_b) MTG_DIE("mtg_compare_kmer_sets_stores: null argument");
    const UnitigStore &a = *store_a->s, &b = *store_b->s;
    device_compare_kmer_sets(a.data.data(), a.off.data(), a.off.size() - 1, b.data.data(), b.off.data(), b.off.size() - 1, k, device_id, out,
                             &g_last_kmer_compare);
}
void mtg_read_sequences(const char *path, mtg_unitigs **store_out) {
    if (!path || !store_out) MTG_DIE("mtg_read_sequences: null argument");
    *store_out = new mtg_unitigs{read_fasta_records(path)};
}
void mtg_last_kmer_compare_times(double out[6]) {
    const KmerCompareTimes &t = g_last_kmer_compare;
    out[0] = t.upload_ms; out[1] = t.pack_ms; out[2] = t.insert_a_ms; out[3] = t.insert_b_ms; out[4] = t.count_ms; out[5] = t.total_ms;
}
// ---- k-mer index on the GPU (kmer_query_device.hip) ----
struct mtg_kmer_index { KmerIndex *ix; };
static thread_local KmerQueryTimes g_last_kmer_query;
mtg_kmer_index *mtg_kmer_index_build(const char *seq, const uint64_t *off, uint64_t n, uint64_t k, int device_id) {
    return new mtg_kmer_index{device_kmer_index_build(seq, off, n, k, device_id, false, &g_last_kmer_query)};
}
mtg_kmer_index *mtg_kmer_index_build_store(const mtg_unitigs *store, uint64_t k, int device_id) {
    if (!store) MTG_DIE("mtg_kmer_index_build_store: null argument");
    const UnitigStore &s = *store->s;
    return new mtg_kmer_index{device_kmer_index_build(s.data.data(), s.off.data(), s.off.size() - 1, k, device_id, false, &g_last_kmer_query)};
}
void mtg_kmer_index_get_info(const mtg_kmer_index *ix, mtg_kmer_index_info *out) {
    if (!ix || !out) MTG_DIE("mtg_kmer_index_get_info: null argument");
    device_kmer_index_info(ix->ix, out);
}
void mtg_kmer_index_query(const mtg_kmer_index *ix, const char *seq, const uint64_t *off, uint64_t n, uint64_t *kmers, uint64_t *valid,
                          uint64_t *found, uint64_t *present_bits, uint64_t *valid_bits) {
    if (!ix) MTG_DIE("mtg_kmer_index_query: null argument");
    device_kmer_index_query(ix->ix, seq, off, n, kmers, valid, found, present_bits, valid_bits, &g_last_kmer_query);
}
void mtg_kmer_index_free(mtg_kmer_index *ix) {
    if (!ix) return;
    device_kmer_index_free(ix->ix);
    delete ix;
}
// ---- ... that also says where its k-mers are ----
struct mtg_kmer_runs { KmerRuns r; };
static thread_local KmerLocateTimes g_last_kmer_locate;
mtg_kmer_index *mtg_kmer_index_build_locating(const char *seq, const uint64_t *off, uint64_t n, uint64_t k, int device_id) {
    return new mtg_kmer_index{device_kmer_index_build(seq, off, n, k, device_id, true, &g_last_kmer_query)};
}
mtg_kmer_index *mtg_kmer_index_build_locating_store(const mtg_unitigs *store, uint64_t k, int device_id) {
    if (!store) MTG_DIE("mtg_kmer_index_build_locating_store: null argument");
    const UnitigStore &s = *store->s;
    return new mtg_kmer_index{device_kmer_index_build(s.data.data(), s.off.data(), s.off.size() - 1, k, device_id, true, &g_last_kmer_query)};
}
int mtg_kmer_index_is_locating(const mtg_kmer_index *ix) {
    if (!ix) MTG_DIE("mtg_kmer_index_is_locating: null argument");
    return device_kmer_index_is_locating(ix->ix) ? 1 : 0;
}
void mtg_kmer_index_locate(const mtg_kmer_index *ix, const char *seq, const uint64_t *off, uint64_t n, uint64_t *kmers, uint64_t *valid,
                           uint64_t *found, mtg_kmer_runs **out) {
    if (!ix || !out) MTG_DIE("mtg_kmer_index_locate: null argument");
    mtg_kmer_runs *runs = new mtg_kmer_runs();
    device_kmer_index_locate(ix->ix, seq, off, n, kmers, valid, found, &runs->r, &g_last_kmer_locate);
    *out = runs;
}
uint64_t mtg_kmer_runs_count(const mtg_kmer_runs *runs) {
    if (!runs) MTG_DIE("mtg_kmer_runs_count: null argument");
    return runs->r.kmers.size();
}
void mtg_kmer_runs_arrays(const mtg_kmer_runs *runs, const uint64_t **q_record, const uint64_t **q_start, const uint64_t **kmers,
                          const uint8_t **strand, const uint64_t **t_record, const uint64_t **t_start) {
    if (!runs || !q_record || !q_start || !kmers || !strand || !t_record || !t_start) MTG_DIE("mtg_kmer_runs_arrays: null argument");
    *q_record = runs->r.q_record.data(); *q_start = runs->r.q_start.data(); *kmers = runs->r.kmers.data();
    *strand = runs->r.strand.data(); *t_record = runs->r.t_record.data(); *t_start = runs->r.t_start.data();
}
void mtg_kmer_runs_free(mtg_kmer_runs *runs) { delete runs; }
void mtg_last_kmer_locate_times(double out[4]) {
    const KmerLocateTimes &t = g_last_kmer_locate;
    out[0] = t.upload_ms; out[1] = t.pack_ms; out[2] = t.probe_ms; out[3] = t.runs_ms;
}
// ---- ... and how heavy they are ----
static thread_local KmerAbundanceTimes g_last_kmer_abundance;
mtg_kmer_index *mtg_kmer_index_build_weighted(const char *seq, const uint64_t *off, uint64_t n, uint64_t k, const uint32_t *weights,
                                              uint64_t n_weights, int locating, int device_id) {
    const KmerWeights w{weights, n_weights};
    return new mtg_kmer_index{device_kmer_index_build(seq, off, n, k, device_id, locating != 0, &g_last_kmer_query, &w)};
}
mtg_kmer_index *mtg_kmer_index_build_weighted_store(const mtg_unitigs *store, uint64_t k, const uint32_t *weights, uint64_t n_weights,
                                                    int locating, int device_id) {
    if (!store) MTG_DIE("mtg_kmer_index_build_weighted_store: null argument");
    const UnitigStore &s = *store->s;
    return mtg_kmer_index_build_weighted(s.data.data(), s.off.data(), s.off.size() - 1, k, weights, n_weights, locating, device_id);
}
int mtg_kmer_index_is_weighted(const mtg_kmer_index *ix) {
    if (!ix) MTG_DIE("mtg_kmer_index_is_weighted: null argument");
    return device_kmer_index_is_weighted(ix->ix) ? 1 : 0;
}
void mtg_kmer_index_abundance(const mtg_kmer_index *ix, const char *seq, const uint64_t *off, uint64_t n, uint64_t *kmers, uint64_t *valid,
                              uint64_t *found, uint64_t *sum, uint32_t *min, uint32_t *max, uint32_t *per_window) {
    if (!ix) MTG_DIE("mtg_kmer_index_abundance: null argument");
    device_kmer_index_abundance(ix->ix, seq, off, n, kmers, valid, found, sum, min, max, per_window, &g_last_kmer_abundance);
}
void mtg_last_kmer_abundance_times(double out[4]) {
    const KmerAbundanceTimes &t = g_last_kmer_abundance;
    out[0] = t.upload_ms; out[1] = t.pack_ms; out[2] = t.probe_ms; out[3] = t.download_ms;
}
// ---- ... and which inputs carry them ----
static thread_local KmerColorTimes g_last_kmer_color;
mtg_kmer_index *mtg_kmer_index_build_annotated(const char *seq, const uint64_t *off, uint64_t n, uint64_t k, const uint32_t *weights,
                                               uint64_t n_weights, const uint64_t *colors, uint64_t n_color_words, uint64_t n_colors,
                                               int locating, int device_id) {
    if (!weights && n_weights) MTG_DIE("mtg_kmer_index_build_annotated: %llu weights but no array", (unsigned long long)n_weights);
    if (!colors && n_color_words) MTG_DIE("mtg_kmer_index_build_annotated: %llu colour words but no array", (unsigned long long)n_color_words);
    const KmerWeights w{weights, n_weights};
    const KmerColors c{colors, n_color_words, n_colors};
    return new mtg_kmer_index{device_kmer_index_build(seq, off, n, k, device_id, locating != 0, &g_last_kmer_query, weights ? &w : nullptr,
                                                      colors ? &c : nullptr)};
}
mtg_kmer_index *mtg_kmer_index_build_annotated_store(const mtg_unitigs *store, uint64_t k, const uint32_t *weights, uint64_t n_weights,
                                                     const uint64_t *colors, uint64_t n_color_words, uint64_t n_colors, int locating,
                                                     int device_id) {
    if (!store) MTG_DIE("mtg_kmer_index_build_annotated_store: null argument");
    const UnitigStore &s = *store->s;
    return mtg_kmer_index_build_annotated(s.data.data(), s.off.data(), s.off.size() - 1, k, weights, n_weights, colors, n_color_words, n_colors,
                                          locating, device_id);
}
int mtg_kmer_index_is_colored(const mtg_kmer_index *ix) {
    if (!ix) MTG_DIE("mtg_kmer_index_is_colored: null argument");
    return device_kmer_index_n_colors(ix->ix) ? 1 : 0;
}
uint64_t mtg_kmer_index_n_colors(const mtg_kmer_index *ix) {
    if (!ix) MTG_DIE("mtg_kmer_index_n_colors: null argument");
    return device_kmer_index_n_colors(ix->ix);
}
void mtg_kmer_index_colors(const mtg_kmer_index *ix, const char *seq, const uint64_t *off, uint64_t n, uint64_t *kmers, uint64_t *valid,
                           uint64_t *found, uint32_t *per_color, uint64_t *per_window) {
    if (!ix) MTG_DIE("mtg_kmer_index_colors: null argument");
    device_kmer_index_colors(ix->ix, seq, off, n, kmers, valid, found, per_color, per_window, &g_last_kmer_color);
}
void mtg_last_kmer_color_times(double out[5]) {
    const KmerColorTimes &t = g_last_kmer_color;
    out[0] = t.stats_ms; out[1] = t.upload_ms; out[2] = t.pack_ms; out[3] = t.probe_ms; out[4] = t.download_ms;
}
// ---- ... and how often other sequences see them ----
struct mtg_kmer_tally { KmerTally *t; };
static thread_local KmerTallyTimes g_last_kmer_tally;
mtg_kmer_tally *mtg_kmer_tally_create(const mtg_kmer_index *ix) {
    if (!ix) MTG_DIE("mtg_kmer_tally_create: null argument");
    return new mtg_kmer_tally{device_kmer_tally_create(ix->ix)};
}
uint64_t mtg_kmer_tally_device_bytes(const mtg_kmer_tally *t) {
    if (!t) MTG_DIE("mtg_kmer_tally_device_bytes: null argument");
    return device_kmer_tally_device_bytes(t->t);
}
void mtg_kmer_tally_add(mtg_kmer_tally *t, const char *seq, const uint64_t *off, uint64_t n, uint64_t *kmers, uint64_t *valid,
                        uint64_t *found) {
    if (!t) MTG_DIE("mtg_kmer_tally_add: null argument");
    device_kmer_tally_add(t->t, seq, off, n, kmers, valid, found, &g_last_kmer_tally);
}
void mtg_kmer_tally_add_store(mtg_kmer_tally *t, const mtg_unitigs *store, uint64_t *kmers, uint64_t *valid, uint64_t *found) {
    if (!t || !store) MTG_DIE("mtg_kmer_tally_add_store: null argument");
    const UnitigStore &s = *store->s;
    mtg_kmer_tally_add(t, s.data.data(), s.off.data(), s.off.size() - 1, kmers, valid, found);
}
void mtg_kmer_tally_coverage(const mtg_kmer_tally *t, const char *seq, const uint64_t *off, uint64_t n, uint64_t *kmers, uint64_t *valid,
                             uint64_t *found, uint64_t *covered, uint64_t *sum, uint64_t *max, uint64_t *per_window) {
    if (!t) MTG_DIE("mtg_kmer_tally_coverage: null argument");
    device_kmer_tally_coverage(t->t, seq, off, n, kmers, valid, found, covered, sum, max, per_window, &g_last_kmer_tally);
}
void mtg_kmer_tally_coverage_store(const mtg_kmer_tally *t, const mtg_unitigs *store, uint64_t *kmers, uint64_t *valid, uint64_t *found,
                                   uint64_t *covered, uint64_t *sum, uint64_t *max, uint64_t *per_window) {
    if (!t || !store) MTG_DIE("mtg_kmer_tally_coverage_store: null argument");
    const UnitigStore &s = *store->s;
    mtg_kmer_tally_coverage(t, s.data.data(), s.off.data(), s.off.size() - 1, kmers, valid, found, covered, sum, max, per_window);
}
void mtg_kmer_tally_reset(mtg_kmer_tally *t) {
    if (!t) MTG_DIE("mtg_kmer_tally_reset: null argument");
    device_kmer_tally_reset(t->t);
}
void mtg_kmer_tally_free(mtg_kmer_tally *t) {
    if (!t) return;
    device_kmer_tally_free(t->t);
    delete t;
}
void mtg_last_kmer_tally_times(double out[4]) {
    const KmerTallyTimes &t = g_last_kmer_tally;
    out[0] = t.upload_ms; out[1] = t.pack_ms; out[2] = t.probe_ms; out[3] = t.download_ms;
}
void mtg_last_kmer_query_times(double out[6]) {
    const KmerQueryTimes &t = g_last_kmer_query;
    out[0] = t.build_upload_ms; out[1] = t.build_pack_ms; out[2] = t.build_insert_ms;
    out[3] = t.query_upload_ms; out[4] = t.query_pack_ms; out[5] = t.query_probe_ms;
}
// ---- the sparse minimizer index (tig_index_device.hip) ----
struct mtg_tig_index {
    TigIndex *ix;
    std::string meta{};  // the metadata blob of the file it was loaded from, or of its last save
};
static thread_local TigIndexTimes g_last_tig_index;
mtg_tig_index *mtg_tig_index_build(const char *seq, const uint64_t *off, uint64_t n, uint64_t k, uint64_t m, uint64_t bucket_limit, int device_id) {
    return new mtg_tig_index{device_tig_index_build(seq, off, n, k, m, bucket_limit, device_id, &g_last_tig_index)};
}
mtg_tig_index *mtg_tig_index_build_store(const mtg_unitigs *store, uint64_t k, uint64_t m, uint64_t bucket_limit, int device_id) {
    if (!store) MTG_DIE("mtg_tig_index_build_store: null argument");
    const UnitigStore &s = *store->s;
    return mtg_tig_index_build(s.data.data(), s.off.data(), s.off.size() - 1, k, m, bucket_limit, device_id);
}
void mtg_tig_index_get_info(const mtg_tig_index *ix, mtg_tig_index_info *out) {
    if (!ix || !out) MTG_DIE("mtg_tig_index_get_info: null argument");
    device_tig_index_info(ix->ix, out);
}
void mtg_tig_index_query(const mtg_tig_index *ix, const char *seq, const uint64_t *off, uint64_t n, uint64_t *kmers, uint64_t *valid,
                         uint64_t *found, uint64_t *present_bits, uint64_t *valid_bits) {
    if (!ix) MTG_DIE("mtg_tig_index_query: null argument");
    device_tig_index_query(ix->ix, seq, off, n, kmers, valid, found, present_bits, valid_bits, &g_last_tig_index);
}
// ---- ... that also says where its k-mers are ----
static thread_local KmerLocateTimes g_last_tig_locate;
mtg_tig_index *mtg_tig_index_build_locating(const char *seq, const uint64_t *off, uint64_t n, uint64_t k, uint64_t m, uint64_t bucket_limit,
                                            int device_id) {
    return new mtg_tig_index{device_tig_index_build(seq, off, n, k, m, bucket_limit, device_id, &g_last_tig_index, true)};
}
mtg_tig_index *mtg_tig_index_build_locating_store(const mtg_unitigs *store, uint64_t k, uint64_t m, uint64_t bucket_limit, int device_id) {
    if (!store) MTG_DIE("mtg_tig_index_build_locating_store: null argument");
    const UnitigStore &s = *store->s;
    return mtg_tig_index_build_locating(s.data.data(), s.off.data(), s.off.size() - 1, k, m, bucket_limit, device_id);
}
int mtg_tig_index_is_locating(const mtg_tig_index *ix) {
    if (!ix) MTG_DIE("mtg_tig_index_is_locating: null argument");
    return device_tig_index_is_locating(ix->ix) ? 1 : 0;
}
void mtg_tig_index_locate(const mtg_tig_index *ix, const char *seq, const uint64_t *off, uint64_t n, uint64_t *kmers, uint64_t *valid,
                          uint64_t *found, mtg_kmer_runs **out) {
    if (!ix || !out) MTG_DIE("mtg_tig_index_locate: null argument");
    mtg_kmer_runs *runs = new mtg_kmer_runs();
    device_tig_index_locate(ix->ix, seq, off, n, kmers, valid, found, &runs->r, &g_last_tig_locate);
    *out = runs;
}
void mtg_last_tig_locate_times(double out[4]) {
    const KmerLocateTimes &t = g_last_tig_locate;
    out[0] = t.upload_ms; out[1] = t.pack_ms; out[2] = t.probe_ms; out[3] = t.runs_ms;
}
// ---- ... and which path through the indexed records a query takes: walks, and their GAF text ----
struct mtg_kmer_walks { KmerWalks w; };
static thread_local KmerThreadTimes g_last_kmer_thread, g_last_tig_thread;
void mtg_kmer_index_thread(const mtg_kmer_index *ix, const char *seq, const uint64_t *off, uint64_t n, uint64_t min_kmers, uint64_t *kmers,
                           uint64_t *valid, uint64_t *found, mtg_kmer_walks **out) {
    if (!ix || !out) MTG_DIE("mtg_kmer_index_thread: null argument");
    std::unique_ptr<mtg_kmer_walks> walks(new mtg_kmer_walks());
    device_kmer_index_thread(ix->ix, seq, off, n, min_kmers, kmers, valid, found, &walks->w, &g_last_kmer_thread);
    *out = walks.release();
}
void mtg_tig_index_thread(const mtg_tig_index *ix, const char *seq, const uint64_t *off, uint64_t n, uint64_t min_kmers, uint64_t *kmers,
                          uint64_t *valid, uint64_t *found, mtg_kmer_walks **out) {
    if (!ix || !out) MTG_DIE("mtg_tig_index_thread: null argument");
    std::unique_ptr<mtg_kmer_walks> walks(new mtg_kmer_walks());
    device_tig_index_thread(ix->ix, seq, off, n, min_kmers, kmers, valid, found, &walks->w, &g_last_tig_thread);
    *out = walks.release();
}
uint64_t mtg_kmer_walks_count(const mtg_kmer_walks *walks) {
    if (!walks) MTG_DIE("mtg_kmer_walks_count: null argument");
    return walks->w.n;
}
uint64_t mtg_kmer_walks_steps_count(const mtg_kmer_walks *walks) {
    if (!walks) MTG_DIE("mtg_kmer_walks_steps_count: null argument");
    return walks->w.steps.size();
}
void mtg_kmer_walks_arrays(const mtg_kmer_walks *walks, const uint64_t *fields[9]) {
    if (!walks || !fields) MTG_DIE("mtg_kmer_walks_arrays: null argument");
    for (int f = 0; f < 9; f++) fields[f] = walks->w.fields.data() + (uint64_t)f * walks->w.n;
}
const uint64_t *mtg_kmer_walks_steps(const mtg_kmer_walks *walks) {
    if (!walks) MTG_DIE("mtg_kmer_walks_steps: null argument");
    return walks->w.steps.data();
}
void mtg_kmer_walks_free(mtg_kmer_walks *walks) { delete walks; }
static void thread_times_out(const KmerThreadTimes &t, double out[5]) {
    out[0] = t.upload_ms; out[1] = t.pack_ms; out[2] = t.probe_ms; out[3] = t.runs_ms; out[4] = t.walks_ms;
}
void mtg_last_kmer_thread_times(double out[5]) { thread_times_out(g_last_kmer_thread, out); }
void mtg_last_tig_thread_times(double out[5]) { thread_times_out(g_last_tig_thread, out); }
// The GAF text is made on the host: a line is names and decimal numbers, a few dozen bytes per step, and the walks are on the host
// already. Two passes over ranges of walks on the host's threads -- the bytes of every line, then the lines at their offsets.
namespace {
struct GafNames {
    const char *text;
    const uint64_t *off;
    uint64_t n;
};
inline size_t put_u64(char *p, uint64_t v) {
    char tmp[20];
    size_t n = 0;
    do tmp[n++] = (char)('0' + v % 10); while (v /= 10);
    for (size_t i = 0; i < n; i++) p[i] = tmp[n - 1 - i];
    return n;
}
inline size_t digits(uint64_t v) {
    size_t n = 1;
    while (v >= 10) { v /= 10; n++; }
    return n;
}
// one line, written at p if p is given; returns its bytes
size_t gaf_line(const KmerWalks &w, uint64_t i, const GafNames &q, const uint64_t *q_len, const GafNames &s, char *p) {
    const uint64_t n = w.n, *f = w.fields.data();
    const uint64_t qr = f[i], qs = f[n + i], qe = f[2 * n + i], kmers = f[3 * n + i], steps = f[4 * n + i], s0 = f[5 * n + i];
    const uint64_t nums[] = {q_len[qr], qs, qe};
    const uint64_t tail[] = {f[6 * n + i], f[7 * n + i], f[8 * n + i], qe - qs, qe - qs};
    size_t b = 0;
    auto text = [&](const char *t, size_t len) { if (p) memcpy(p + b, t, len); b += len; };
    auto num = [&](uint64_t v) { b += p ? put_u64(p + b, v) : digits(v); };
    auto chr = [&](char c) { if (p) p[b] = c; b++; };
    text(q.text + q.off[qr], q.off[qr + 1] - q.off[qr]);
    for (uint64_t v : nums) { chr('\t'); num(v); }
    text("\t+\t", 3);
    for (uint64_t j = 0; j < steps; j++) {
        const uint64_t st = w.steps[s0 + j], u = st >> 1;
        chr((st & 1) ? '<' : '>');
        if (s.text) text(s.text + s.off[u], s.off[u + 1] - s.off[u]);
        else num(u);
    }
    for (uint64_t v : tail) { chr('\t'); num(v); }
    text("\t255\tcg:Z:", 10);
    num(qe - qs);
    text("=\tkm:i:", 7);
    num(kmers);
    chr('\n');
    return b;
}
}  // namespace
uint64_t mtg_kmer_walks_gaf(const mtg_kmer_walks *walks, uint64_t n_queries, const char *query_names, const uint64_t *query_name_off,
                            const uint64_t *query_len, uint64_t n_segments, const char *segment_names, const uint64_t *segment_name_off,
                            char **text_out) {
    const char *fn = "mtg_kmer_walks_gaf";
    if (!walks || !text_out || (n_queries && (!query_name_off || !query_len)) || (segment_names && !segment_name_off)) MTG_DIE("%s: null argument", fn);
    const KmerWalks &w = walks->w;
    const uint64_t n = w.n;
    for (uint64_t i = 0; i < n; i++)
        if (w.fields[i] >= n_queries) MTG_DIE("%s: walk %llu is of query record %llu; %llu names", fn, (unsigned long long)i, (unsigned long long)w.fields[i], (unsigned long long)n_queries);
    if (segment_names)
        for (uint64_t st : w.steps)
            if ((st >> 1) >= n_segments) MTG_DIE("%s: a step on segment %llu; %llu names", fn, (unsigned long long)(st >> 1), (unsigned long long)n_segments);
    const GafNames q{query_names ? query_names : "", query_name_off, n_queries}, s{segment_names, segment_name_off, n_segments};
    constexpr uint64_t CHUNK = 4096;  // walks per task
    const uint64_t chunks = (n + CHUNK - 1) / CHUNK;
    std::vector<uint64_t> at(chunks + 1, 0);
    parallel_tasks(chunks, [&](uint64_t c) {
        uint64_t b = 0;
        for (uint64_t i = c * CHUNK; i < std::min(n, (c + 1) * CHUNK); i++) b += gaf_line(w, i, q, query_len, s, nullptr);
        at[c + 1] = b;
    });
    for (uint64_t c = 0; c < chunks; c++) at[c + 1] += at[c];
    char *text = (char *)malloc(at[chunks] + 1);
    if (!text) MTG_DIE("%s: out of memory (%llu bytes)", fn, (unsigned long long)at[chunks]);
    parallel_tasks(chunks, [&](uint64_t c) {
        char *p = text + at[c];
        for (uint64_t i = c * CHUNK; i < std::min(n, (c + 1) * CHUNK); i++) p += gaf_line(w, i, q, query_len, s, p);
    });
    text[at[chunks]] = 0;
    *text_out = text;
    return at[chunks];
}
// ---- ... and how heavy they are and which inputs carry them: payloads by position ----
static thread_local TigPayloadTimes g_last_tig_payload;
mtg_tig_index *mtg_tig_index_build_annotated(const char *seq, const uint64_t *off, uint64_t n, uint64_t k, uint64_t m, uint64_t bucket_limit,
                                             const uint32_t *weights, uint64_t n_weights, const uint64_t *colors, uint64_t n_color_words,
                                             uint64_t n_colors, int layout, int device_id) {
    if (!weights && n_weights) MTG_DIE("mtg_tig_index_build_annotated: %llu weights but no array", (unsigned long long)n_weights);
    if (!colors && n_color_words) MTG_DIE("mtg_tig_index_build_annotated: %llu colour words but no array", (unsigned long long)n_color_words);
    const KmerWeights w{weights, n_weights};
    const KmerColors c{colors, n_color_words, n_colors};
    return new mtg_tig_index{device_tig_index_build_annotated(seq, off, n, k, m, bucket_limit, weights ? &w : nullptr, colors ? &c : nullptr, layout,
                                                              device_id, &g_last_tig_index, &g_last_tig_payload)};
}
mtg_tig_index *mtg_tig_index_build_annotated_store(const mtg_unitigs *store, uint64_t k, uint64_t m, uint64_t bucket_limit,
                                                   const uint32_t *weights, uint64_t n_weights, const uint64_t *colors,
                                                   uint64_t n_color_words, uint64_t n_colors, int layout, int device_id) {
    if (!store) MTG_DIE("mtg_tig_index_build_annotated_store: null argument");
    const UnitigStore &s = *store->s;
    return mtg_tig_index_build_annotated(s.data.data(), s.off.data(), s.off.size() - 1, k, m, bucket_limit, weights, n_weights, colors,
                                         n_color_words, n_colors, layout, device_id);
}
void mtg_tig_index_get_payload_info(const mtg_tig_index *ix, mtg_tig_payload_info *out) {
    if (!ix || !out) MTG_DIE("mtg_tig_index_get_payload_info: null argument");
    device_tig_index_payload_info(ix->ix, out);
}
int mtg_tig_index_is_weighted(const mtg_tig_index *ix) {
    if (!ix) MTG_DIE("mtg_tig_index_is_weighted: null argument");
    mtg_tig_payload_info info;
    device_tig_index_payload_info(ix->ix, &info);
    return info.weights.layout ? 1 : 0;
}
int mtg_tig_index_is_colored(const mtg_tig_index *ix) {
    if (!ix) MTG_DIE("mtg_tig_index_is_colored: null argument");
    mtg_tig_payload_info info;
    device_tig_index_payload_info(ix->ix, &info);
    return info.colors.layout ? 1 : 0;
}
void mtg_tig_index_abundance(const mtg_tig_index *ix, const char *seq, const uint64_t *off, uint64_t n, uint64_t *kmers, uint64_t *valid,
                             uint64_t *found, uint64_t *sum, uint32_t *min, uint32_t *max, uint32_t *per_window) {
    if (!ix) MTG_DIE("mtg_tig_index_abundance: null argument");
    device_tig_index_abundance(ix->ix, seq, off, n, kmers, valid, found, sum, min, max, per_window, &g_last_tig_payload);
}
void mtg_tig_index_colors(const mtg_tig_index *ix, const char *seq, const uint64_t *off, uint64_t n, uint64_t *kmers, uint64_t *valid,
                          uint64_t *found, uint32_t *per_color, uint64_t *per_window) {
    if (!ix) MTG_DIE("mtg_tig_index_colors: null argument");
    device_tig_index_colors(ix->ix, seq, off, n, kmers, valid, found, per_color, per_window, &g_last_tig_payload);
}
void mtg_last_tig_payload_times(double out[12]) {
    const TigPayloadTimes &t = g_last_tig_payload;
    for (int i = 0; i < 4; i++) {
        out[i] = t.weights_ms[i];
        out[4 + i] = t.colors_ms[i];
    }
    out[8] = t.upload_ms; out[9] = t.pack_ms; out[10] = t.probe_ms; out[11] = t.gather_ms;
}
// ---- tallies by position on the sparse index (tig_tally_device.hpp) ----
struct mtg_tig_tally { TigTally *t; };
static thread_local TigTallyTimes g_last_tig_tally;
mtg_tig_tally *mtg_tig_tally_create(const mtg_tig_index *ix) {
    if (!ix) MTG_DIE("mtg_tig_tally_create: null argument");
    return new mtg_tig_tally{device_tig_tally_create(ix->ix)};
}
uint64_t mtg_tig_tally_device_bytes(const mtg_tig_tally *t) {
    if (!t) MTG_DIE("mtg_tig_tally_device_bytes: null argument");
    return device_tig_tally_device_bytes(t->t);
}
uint64_t mtg_tig_tally_windows(const mtg_tig_tally *t) {
    if (!t) MTG_DIE("mtg_tig_tally_windows: null argument");
    return device_tig_tally_windows(t->t);
}
void mtg_tig_tally_add(mtg_tig_tally *t, const char *seq, const uint64_t *off, uint64_t n, uint64_t *kmers, uint64_t *valid, uint64_t *found) {
    if (!t) MTG_DIE("mtg_tig_tally_add: null argument");
    device_tig_tally_add(t->t, seq, off, n, kmers, valid, found, &g_last_tig_tally);
}
void mtg_tig_tally_add_store(mtg_tig_tally *t, const mtg_unitigs *store, uint64_t *kmers, uint64_t *valid, uint64_t *found) {
    if (!t || !store) MTG_DIE("mtg_tig_tally_add_store: null argument");
    const UnitigStore &s = *store->s;
    mtg_tig_tally_add(t, s.data.data(), s.off.data(), s.off.size() - 1, kmers, valid, found);
}
void mtg_tig_tally_coverage(const mtg_tig_tally *t, const char *seq, const uint64_t *off, uint64_t n, uint64_t *kmers, uint64_t *valid,
                            uint64_t *found, uint64_t *covered, uint64_t *sum, uint64_t *max, uint64_t *per_window) {
    if (!t) MTG_DIE("mtg_tig_tally_coverage: null argument");
    device_tig_tally_coverage(t->t, seq, off, n, kmers, valid, found, covered, sum, max, per_window, &g_last_tig_tally);
}
void mtg_tig_tally_coverage_store(const mtg_tig_tally *t, const mtg_unitigs *store, uint64_t *kmers, uint64_t *valid, uint64_t *found,
                                  uint64_t *covered, uint64_t *sum, uint64_t *max, uint64_t *per_window) {
    if (!t || !store) MTG_DIE("mtg_tig_tally_coverage_store: null argument");
    const UnitigStore &s = *store->s;
    mtg_tig_tally_coverage(t, s.data.data(), s.off.data(), s.off.size() - 1, kmers, valid, found, covered, sum, max, per_window);
}
void mtg_tig_tally_counters(const mtg_tig_tally *t, uint64_t *out) {
    if (!t) MTG_DIE("mtg_tig_tally_counters: null argument");
    device_tig_tally_counters(t->t, out);
}
void mtg_tig_tally_reset(mtg_tig_tally *t) {
    if (!t) MTG_DIE("mtg_tig_tally_reset: null argument");
    device_tig_tally_reset(t->t);
}
void mtg_tig_tally_free(mtg_tig_tally *t) {
    if (!t) return;
    device_tig_tally_free(t->t);
    delete t;
}
void mtg_last_tig_tally_times(double out[5]) {
    const TigTallyTimes &t = g_last_tig_tally;
    out[0] = t.upload_ms; out[1] = t.pack_ms; out[2] = t.probe_ms; out[3] = t.pass2_ms; out[4] = t.download_ms;
}
// ---- pseudoalignment with equivalence classes on either coloured index (pseudoalign_device.hpp) ----
// The aligner is host state only: the rule, the dictionary of the masks seen so far and the totals. A call's device work is transient.
struct mtg_pseudoaligner {
    const KmerIndex *table;  // one of the two
    const TigIndex *sparse;
    PseudoalignRule rule;
    struct Class { uint64_t mask, fragments, first; };
    std::vector<Class> classes;  // (in no particular order: mtg_pseudoaligner_classes sorts)
    uint64_t totals[4] = {0, 0, 0, 0};
};
static thread_local PseudoalignCall g_last_pseudoalign;
static mtg_pseudoaligner *pseudoaligner_new(const char *fn, const KmerIndex *table, const TigIndex *sparse, const mtg_pseudoalign_params *p) {
    const mtg_pseudoalign_params q = p ? *p : mtg_pseudoalign_params{1000, 0, 1};
    const uint64_t C = table ? device_kmer_index_n_colors(table) : device_tig_index_n_colors(sparse);
    if (!C) MTG_DIE("%s: the index keeps no colours (build it with %s)", fn, table ? "mtg_kmer_index_build_annotated" : "mtg_tig_index_build_annotated");
    if (q.threshold_permille < 1 || q.threshold_permille > 1000)
        MTG_DIE("%s: threshold_permille %llu is outside 1 .. 1000", fn, (unsigned long long)q.threshold_permille);
    if (q.min_kmers < 1) MTG_DIE("%s: min_kmers must be >= 1", fn);
    return new mtg_pseudoaligner{table, sparse, PseudoalignRule{q.threshold_permille, q.min_kmers, q.over_valid ? 1u : 0u}, {}, {0, 0, 0, 0}};
}
mtg_pseudoaligner *mtg_pseudoaligner_create(const mtg_kmer_index *ix, const mtg_pseudoalign_params *p) {
    if (!ix) MTG_DIE("mtg_pseudoaligner_create: null argument");
    return pseudoaligner_new("mtg_pseudoaligner_create", ix->ix, nullptr, p);
}
mtg_pseudoaligner *mtg_pseudoaligner_create_tig(const mtg_tig_index *ix, const mtg_pseudoalign_params *p) {
    if (!ix) MTG_DIE("mtg_pseudoaligner_create_tig: null argument");
    return pseudoaligner_new("mtg_pseudoaligner_create_tig", nullptr, ix->ix, p);
}
void mtg_pseudoaligner_align(mtg_pseudoaligner *pa, const char *seq, const uint64_t *off, uint64_t n, const char *mate_seq, const uint64_t *mate_off,
                             uint64_t *kmers, uint64_t *valid, uint64_t *found, uint64_t *masks) {
    if (!pa) MTG_DIE("mtg_pseudoaligner_align: null argument");
    if ((mate_seq == nullptr) != (mate_off == nullptr)) MTG_DIE("mtg_pseudoaligner_align: mate_seq and mate_off go together (both NULL: single-end)");
    g_last_pseudoalign = PseudoalignCall();
    if (n == 0) return;
    PseudoalignCall &call = g_last_pseudoalign;
    if (pa->table) device_kmer_index_pseudoalign(pa->table, pa->rule, pa->totals[0], seq, off, n, mate_seq, mate_off, kmers, valid, found, masks, &call);
    else device_tig_index_pseudoalign(pa->sparse, pa->rule, pa->totals[0], seq, off, n, mate_seq, mate_off, kmers, valid, found, masks, &call);
    // the call's classes into the aligner's (a few masks as a rule: a sorted copy of the keys, then a binary search per class)
    std::vector<std::pair<uint64_t, size_t>> known(pa->classes.size());
    for (size_t i = 0; i < known.size(); i++) known[i] = {pa->classes[i].mask, i};
    std::sort(known.begin(), known.end());
    for (size_t i = 0; i < call.mask.size(); i++) {
        auto it = std::lower_bound(known.begin(), known.end(), std::make_pair(call.mask[i], (size_t)0));
        if (it != known.end() && it->first == call.mask[i]) {
            mtg_pseudoaligner::Class &c = pa->classes[it->second];
            c.fragments += call.fragments[i];
            c.first = std::min(c.first, call.first[i]);
        } else {
            pa->classes.push_back({call.mask[i], call.fragments[i], call.first[i]});  // (a call's masks are distinct)
        }
    }
    pa->totals[0] += n;
    pa->totals[1] += call.eligible;
    pa->totals[2] += call.assigned;
    pa->totals[3] += call.ambiguous;
}
void mtg_pseudoaligner_align_store(mtg_pseudoaligner *pa, const mtg_unitigs *reads, const mtg_unitigs *mates, uint64_t *kmers, uint64_t *valid,
                                   uint64_t *found, uint64_t *masks) {
    if (!pa || !reads) MTG_DIE("mtg_pseudoaligner_align_store: null argument");
    const UnitigStore &s = *reads->s;
    const uint64_t n = s.off.size() - 1;
    if (mates && mates->s->off.size() - 1 != n)
        MTG_DIE("mtg_pseudoaligner_align_store: %llu reads and %llu mates", (unsigned long long)n, (unsigned long long)(mates->s->off.size() - 1));
    // (a store without bases may have no data pointer: the mates are told from the offsets)
    static const char none = 0;
    const char *mate_seq = mates ? (mates->s->data.data() ? mates->s->data.data() : &none) : nullptr;
    mtg_pseudoaligner_align(pa, s.data.data(), s.off.data(), n, mate_seq, mates ? mates->s->off.data() : nullptr, kmers, valid, found, masks);
}
uint64_t mtg_pseudoaligner_classes(const mtg_pseudoaligner *pa, uint64_t **mask, uint64_t **fragments, uint64_t **first) {
    if (!pa || !mask || !fragments || !first) MTG_DIE("mtg_pseudoaligner_classes: null argument");
    std::vector<mtg_pseudoaligner::Class> sorted = pa->classes;
    std::sort(sorted.begin(), sorted.end(), [](const mtg_pseudoaligner::Class &a, const mtg_pseudoaligner::Class &b) { return a.first < b.first; });
    const size_t n = sorted.size();
    *mask = *fragments = *first = nullptr;
    if (!n) return 0;
    *mask = (uint64_t *)std::malloc(n * 8);
    *fragments = (uint64_t *)std::malloc(n * 8);
    *first = (uint64_t *)std::malloc(n * 8);
    if (!*mask || !*fragments || !*first) MTG_DIE("mtg_pseudoaligner_classes: out of memory");
    for (size_t i = 0; i < n; i++) {
        (*mask)[i] = sorted[i].mask;
        (*fragments)[i] = sorted[i].fragments;
        (*first)[i] = sorted[i].first;
    }
    return n;
}
void mtg_pseudoaligner_totals(const mtg_pseudoaligner *pa, uint64_t out[4]) {
    if (!pa || !out) MTG_DIE("mtg_pseudoaligner_totals: null argument");
    std::copy(pa->totals, pa->totals + 4, out);
}
void mtg_pseudoaligner_reset(mtg_pseudoaligner *pa) {
    if (!pa) MTG_DIE("mtg_pseudoaligner_reset: null argument");
    pa->classes.clear();
    std::fill(pa->totals, pa->totals + 4, 0ull);
}
void mtg_pseudoaligner_free(mtg_pseudoaligner *pa) { delete pa; }
void mtg_last_pseudoalign_times(double out[6]) {
    const PseudoalignCall &t = g_last_pseudoalign;
    out[0] = t.upload_ms; out[1] = t.pack_ms; out[2] = t.probe_ms; out[3] = t.mask_ms; out[4] = t.dictionary_ms; out[5] = t.download_ms;
}
// ---- read correction against the table index's k-mers (kmer_correct_device.hpp) ----
static thread_local KmerCorrectCall g_last_kmer_correct;
void mtg_kmer_index_correct(const mtg_kmer_index *ix, const char *seq, const uint64_t *off, uint64_t n, const mtg_correct_params *params,
                            uint64_t *kmers, uint64_t *valid, uint64_t *found, uint64_t *found_after, uint64_t *candidates, uint64_t *ambiguous,
                            uint64_t *corrected, uint64_t **positions, uint8_t **bases, uint64_t *n_substitutions, uint64_t round_corrected[8]) {
    const mtg_correct_params q = params ? *params : mtg_correct_params{4, 2};
    if (q.min_solid < 1) MTG_DIE("mtg_kmer_index_correct: min_solid must be >= 1");
    if (q.rounds < 1 || q.rounds > 8) MTG_DIE("mtg_kmer_index_correct: rounds %u is outside 1 .. 8", q.rounds);
    if (!ix || !positions || !bases || !n_substitutions || !round_corrected) MTG_DIE("mtg_kmer_index_correct: null argument");
    g_last_kmer_correct = KmerCorrectCall();
    *positions = nullptr;
    *bases = nullptr;
    *n_substitutions = 0;
    std::fill(round_corrected, round_corrected + 8, 0ull);
    if (n == 0) return;
    KmerCorrectCall &call = g_last_kmer_correct;
    device_kmer_index_correct(ix->ix, q.min_solid, q.rounds, seq, off, n, kmers, valid, found, found_after, candidates, ambiguous, corrected, &call);
    std::copy(call.round_corrected, call.round_corrected + 8, round_corrected);
    const size_t m = call.positions.size();
    *n_substitutions = m;
    if (m) {
        *positions = (uint64_t *)std::malloc(m * 8);
        *bases = (uint8_t *)std::malloc(m);
        if (!*positions || !*bases) MTG_DIE("mtg_kmer_index_correct: out of memory");
        std::copy(call.positions.begin(), call.positions.end(), *positions);
        std::copy(call.bases.begin(), call.bases.end(), *bases);
    }
    call.positions = std::vector<uint64_t>();  // (the times stay for mtg_last_kmer_correct_times)
    call.bases = std::vector<uint8_t>();
}
void mtg_kmer_index_correct_store(const mtg_kmer_index *ix, const mtg_unitigs *reads, const mtg_correct_params *params, uint64_t *kmers,
                                  uint64_t *valid, uint64_t *found, uint64_t *found_after, uint64_t *candidates, uint64_t *ambiguous,
                                  uint64_t *corrected, uint64_t **positions, uint8_t **bases, uint64_t *n_substitutions, uint64_t round_corrected[8]) {
    if (!ix || !reads) MTG_DIE("mtg_kmer_index_correct_store: null argument");
    const UnitigStore &s = *reads->s;
    mtg_kmer_index_correct(ix, s.data.data(), s.off.data(), s.off.size() - 1, params, kmers, valid, found, found_after, candidates, ambiguous,
                           corrected, positions, bases, n_substitutions, round_corrected);
}
void mtg_last_kmer_correct_times(double out[8]) {
    const KmerCorrectCall &t = g_last_kmer_correct;
    out[0] = t.upload_ms; out[1] = t.pack_ms; out[2] = t.query_ms; out[3] = t.flag_ms; out[4] = t.evaluate_ms; out[5] = t.apply_ms;
    out[6] = t.download_ms; out[7] = t.total_ms;
}
// ---- the index as a file ----
static thread_local TigIndexFileTimes g_last_tig_index_file;
static void put_message(const std::string &msg, char *err, uint64_t err_len) {
    if (err && err_len) std::snprintf(err, err_len, "%s", msg.c_str());
}
int mtg_tig_index_save(const mtg_tig_index *ix, const char *path, const char *meta_json, uint64_t meta_len, char *err, uint64_t err_len) {
    if (!ix || !path || (meta_len && !meta_json)) MTG_DIE("mtg_tig_index_save: null argument");
    std::string why;
    if (!device_tig_index_save(ix->ix, path, meta_json, meta_len, &g_last_tig_index_file, why)) {
        put_message(why, err, err_len);
        return 2;
    }
    const_cast<mtg_tig_index *>(ix)->meta.assign(meta_json ? meta_json : "", meta_len);
    return 0;
}
mtg_tig_index *mtg_tig_index_load(const char *path, int device_id, char *err, uint64_t err_len) {
    if (!path) MTG_DIE("mtg_tig_index_load: null argument");
    std::string why, meta;
    TigIndex *t = device_tig_index_load(path, device_id, meta, &g_last_tig_index_file, why);
    if (!t) {
        put_message(why, err, err_len);
        return nullptr;
    }
    mtg_tig_index *ix = new mtg_tig_index{t};
    ix->meta = std::move(meta);
    return ix;
}
const char *mtg_tig_index_meta(const mtg_tig_index *ix, uint64_t *len) {
    if (!ix) MTG_DIE("mtg_tig_index_meta: null argument");
    if (len) *len = ix->meta.size();
    return ix->meta.data();
}
void mtg_last_tig_index_file_times(double out[7]) {
    const TigIndexFileTimes &t = g_last_tig_index_file;
    out[0] = t.save_digest_ms; out[1] = t.save_download_ms; out[2] = t.save_write_ms;
    out[3] = t.load_read_ms; out[4] = t.load_upload_ms; out[5] = t.load_digest_ms; out[6] = t.load_validate_ms;
}
void mtg_tig_index_free(mtg_tig_index *ix) {
    if (!ix) return;
    device_tig_index_free(ix->ix);
    delete ix;
}
void mtg_last_tig_index_times(double out[8]) {
    const TigIndexTimes &t = g_last_tig_index;
    out[0] = t.build_upload_ms; out[1] = t.build_pack_ms; out[2] = t.build_anchors_ms; out[3] = t.build_directory_ms; out[4] = t.build_heavy_ms;
    out[5] = t.query_upload_ms; out[6] = t.query_pack_ms; out[7] = t.query_probe_ms;
}
void mtg_read_sequences_named(const char *path, mtg_unitigs **seqs_out, mtg_unitigs **names_out) {
    if (!path || !seqs_out || !names_out) MTG_DIE("mtg_read_sequences_named: null argument");
    UnitigStore *names = nullptr;
    *seqs_out = new mtg_unitigs{read_fasta_records_named(path, &names)};
    *names_out = new mtg_unitigs{names};
}
// ---- unitig compaction on the GPU (compact_device.hip) ----
static thread_local CompactTimes g_last_compact;
static thread_local ColorClassTimes g_last_color_class;
static thread_local double g_last_clean[2];  // ms of the decision and removal kernels, rounds run
static thread_local double g_last_bubble;    // ms of the bubble kernels over all rounds
struct mtg_abundance_sums { std::vector<uint64_t> v; };
struct mtg_kmer_counts { std::vector<uint32_t> v; };
struct mtg_kmer_colors { std::vector<uint64_t> v; };
struct mtg_color_classes { ColorClasses c; };  // 
// The ladder of the compaction's entry points: each rung takes and hands out what the one below does, and more. A new rung is one
// value here, its fields behind the others in CompactIn / CompactOut and its lines in compact_call.
enum CompactRung { PLAIN, COUNTED, COUNTED_KMERS, COLORED, CLASSES };
struct CompactIn {
    const char *data;
    const uint64_t *offsets;
    uint64_t n, k;
    int device_id;
    uint64_t min_abundance = 1;              // from COUNTED on
    const uint8_t *record_colors = nullptr;  // from COLORED on
    uint64_t n_colors = 0;
    int split = 0;                           // CLASSES
    const mtg_cleaning_params *cleaning = nullptr;  // mtg_compact_unitigs_cleaned, at any rung
    const mtg_bubble_params *bubbles = nullptr;     // mtg_compact_unitigs_simplified, from COUNTED on
    const mtg_selection_params *selection = nullptr;  // mtg_compact_unitigs_selected, from COUNTED on; the filter store: data, offsets, roles
    const char *filter_data = nullptr;
    const uint64_t *filter_offsets = nullptr;
    const uint8_t *filter_roles = nullptr;
    uint64_t filter_n = 0;
};
struct CompactOut {
    mtg_unitigs **out;
    mtg_compaction *stats;
    mtg_abundance *abundance = nullptr;       // from COUNTED on
    mtg_abundance_sums **sums = nullptr;
    mtg_kmer_counts **kmer_counts = nullptr;  // from COUNTED_KMERS on
    mtg_kmer_colors **kmer_colors = nullptr;  // from COLORED on
    mtg_color_stats *color_stats = nullptr;
    mtg_color_classes **classes = nullptr;    // CLASSES
    mtg_cleaning *cleaning = nullptr;         // mtg_compact_unitigs_cleaned
    mtg_bubbles *bubbles = nullptr;           // mtg_compact_unitigs_simplified
    mtg_selection *selection = nullptr;       // mtg_compact_unitigs_selected
};
// what all mtg_compact_unitigs* share: the argument checks, the handles and their way to the out-pointers (who: the entry point)
static void compact_call(const char *who, CompactRung rung, const CompactIn &in, const CompactOut &o) {
    if (!o.out || (rung >= COUNTED && !o.sums) || (rung >= COUNTED_KMERS && !o.kmer_counts) ||
        (rung >= COLORED && (!o.kmer_colors || !o.color_stats)) || (rung >= CLASSES && !o.classes))
        MTG_DIE("%s: null argument", who);
    if (rung >= COUNTED && in.min_abundance == 0) MTG_DIE("%s: min_abundance must be >= 1", who);
    if (rung >= CLASSES && in.split != 0 && in.split != 1) MTG_DIE("%s: split must be 0 or 1, not %d", who, in.split);
    mtg_abundance_sums *s = rung >= COUNTED ? new mtg_abundance_sums() : nullptr;
    mtg_kmer_counts *c = rung >= COUNTED_KMERS ? new mtg_kmer_counts() : nullptr;
    mtg_kmer_colors *m = rung >= COLORED ? new mtg_kmer_colors() : nullptr;
    mtg_color_classes *cl = rung >= CLASSES ? new mtg_color_classes() : nullptr;
    const Counted counted{in.min_abundance, o.abundance, s ? &s->v : nullptr, c ? &c->v : nullptr};
    const Colored colored{in.record_colors, in.n_colors, m ? &m->v : nullptr, o.color_stats, &g_last_kmer_color.stats_ms};
    const Classed classed{in.split == 1, cl ? &cl->c : nullptr, &g_last_color_class};
    mtg_cleaning none{};
    const bool clean = in.cleaning && o.cleaning;
    const Cleaned cleaned{clean ? *in.cleaning : mtg_cleaning_params{0, 0, 1}, clean ? o.cleaning : &none, &g_last_clean[0]};
    mtg_bubbles none_popped{};
    const bool pop = in.bubbles && o.bubbles && in.bubbles->max_arm_kmers;
    if (pop && !clean) MTG_DIE("%s: popping bubbles needs the cleaning parameters (they carry the rounds) and the cleaning out-pointer", who);
    if (pop && rung < COUNTED) MTG_DIE("%s: popping bubbles compares abundances and needs the abundance and sums out-pointers", who);
    const Bubbled bubbled{pop ? *in.bubbles : mtg_bubble_params{0, 1}, pop ? o.bubbles : &none_popped, &g_last_bubble};
    const bool select = in.selection && o.selection;
    if (select && rung < COUNTED) MTG_DIE("%s: a selection reports occurrences and needs the abundance and sums out-pointers", who);
    const Selected selected{select ? *in.selection : mtg_selection_params{0, 0, 0, 64, 1, 1}, in.filter_data, in.filter_offsets, in.filter_roles, in.filter_n,
                            o.selection};
    *o.out = new mtg_unitigs{device_compact_unitigs({who, in.data, in.offsets, in.n, in.k, in.device_id, o.stats, &g_last_compact, s ? &counted : nullptr,
                                                     m ? &colored : nullptr, cl ? &classed : nullptr, &cleaned, &bubbled, select ? &selected : nullptr})};
    g_last_clean[1] = (double)cleaned.out->rounds_run;
    if (o.cleaning && !clean) *o.cleaning = none;
    if (o.bubbles && !pop) *o.bubbles = none_popped;
    if (o.selection && !select) *o.selection = mtg_selection{};
    if (s) *o.sums = s;
    if (c) *o.kmer_counts = c;
    if (m) *o.kmer_colors = m;
    if (cl) *o.classes = cl;
}
void mtg_compact_unitigs(const char *data, const uint64_t *offsets, uint64_t n, uint64_t k, int device_id, mtg_unitigs **out, mtg_compaction *stats) {
    compact_call("mtg_compact_unitigs", PLAIN, {data, offsets, n, k, device_id}, {out, stats});
}
void mtg_compact_unitigs_store(const mtg_unitigs *in, uint64_t k, int device_id, mtg_unitigs **out, mtg_compaction *stats) {
    if (!in || !out) MTG_DIE("mtg_compact_unitigs_store: null argument");
    mtg_compact_unitigs(in->s->data.data(), in->s->off.data(), in->s->off.size() - 1, k, device_id, out, stats);
}
void mtg_compact_unitigs_counted(const char *data, const uint64_t *offsets, uint64_t n, uint64_t k, uint64_t min_abundance, int device_id,
                                 mtg_unitigs **out, mtg_compaction *stats, mtg_abundance *abundance, mtg_abundance_sums **sums) {
    compact_call("mtg_compact_unitigs_counted", COUNTED, {data, offsets, n, k, device_id, min_abundance}, {out, stats, abundance, sums});
}
void mtg_compact_unitigs_counted_store(const mtg_unitigs *in, uint64_t k, uint64_t min_abundance, int device_id, mtg_unitigs **out,
                                       mtg_compaction *stats, mtg_abundance *abundance, mtg_abundance_sums **sums) {
    if (!in) MTG_DIE("mtg_compact_unitigs_counted_store: null argument");
    mtg_compact_unitigs_counted(in->s->data.data(), in->s->off.data(), in->s->off.size() - 1, k, min_abundance, device_id, out, stats, abundance, sums);
}
void mtg_compact_unitigs_counted_kmers(const char *data, const uint64_t *offsets, uint64_t n, uint64_t k, uint64_t min_abundance, int device_id,
                                       mtg_unitigs **out, mtg_compaction *stats, mtg_abundance *abundance, mtg_abundance_sums **sums,
                                       mtg_kmer_counts **kmer_counts) {
    compact_call("mtg_compact_unitigs_counted_kmers", COUNTED_KMERS, {data, offsets, n, k, device_id, min_abundance},
                 {out, stats, abundance, sums, kmer_counts});
}
void mtg_compact_unitigs_counted_kmers_store(const mtg_unitigs *in, uint64_t k, uint64_t min_abundance, int device_id, mtg_unitigs **out,
                                             mtg_compaction *stats, mtg_abundance *abundance, mtg_abundance_sums **sums,
                                             mtg_kmer_counts **kmer_counts) {
    if (!in) MTG_DIE("mtg_compact_unitigs_counted_kmers_store: null argument");
    mtg_compact_unitigs_counted_kmers(in->s->data.data(), in->s->off.data(), in->s->off.size() - 1, k, min_abundance, device_id, out, stats, abundance,
                                      sums, kmer_counts);
}
void mtg_compact_unitigs_colored(const char *data, const uint64_t *offsets, uint64_t n, uint64_t k, uint64_t min_abundance,
                                 const uint8_t *record_colors, uint64_t n_colors, int device_id, mtg_unitigs **out, mtg_compaction *stats,
                                 mtg_abundance *abundance, mtg_abundance_sums **sums, mtg_kmer_counts **kmer_counts,
                                 mtg_kmer_colors **kmer_colors, mtg_color_stats *color_stats) {
    compact_call("mtg_compact_unitigs_colored", COLORED, {data, offsets, n, k, device_id, min_abundance, record_colors, n_colors},
                 {out, stats, abundance, sums, kmer_counts, kmer_colors, color_stats});
}
void mtg_compact_unitigs_colored_store(const mtg_unitigs *in, uint64_t k, uint64_t min_abundance, const uint8_t *record_colors,
                                       uint64_t n_colors, int device_id, mtg_unitigs **out, mtg_compaction *stats, mtg_abundance *abundance,
                                       mtg_abundance_sums **sums, mtg_kmer_counts **kmer_counts, mtg_kmer_colors **kmer_colors,
                                       mtg_color_stats *color_stats) {
    if (!in) MTG_DIE("mtg_compact_unitigs_colored_store: null argument");
    mtg_compact_unitigs_colored(in->s->data.data(), in->s->off.data(), in->s->off.size() - 1, k, min_abundance, record_colors, n_colors, device_id,
                                out, stats, abundance, sums, kmer_counts, kmer_colors, color_stats);
}
void mtg_compact_unitigs_colored_classes(const char *data, const uint64_t *offsets, uint64_t n, uint64_t k, uint64_t min_abundance,
                                         const uint8_t *record_colors, uint64_t n_colors, int split, int device_id, mtg_unitigs **out,
                                         mtg_compaction *stats, mtg_abundance *abundance, mtg_abundance_sums **sums,
                                         mtg_kmer_counts **kmer_counts, mtg_kmer_colors **kmer_colors, mtg_color_stats *color_stats,
                                         mtg_color_classes **classes) {
    compact_call("mtg_compact_unitigs_colored_classes", CLASSES, {data, offsets, n, k, device_id, min_abundance, record_colors, n_colors, split},
                 {out, stats, abundance, sums, kmer_counts, kmer_colors, color_stats, classes});
}
void mtg_compact_unitigs_colored_classes_store(const mtg_unitigs *in, uint64_t k, uint64_t min_abundance, const uint8_t *record_colors,
                                               uint64_t n_colors, int split, int device_id, mtg_unitigs **out, mtg_compaction *stats,
                                               mtg_abundance *abundance, mtg_abundance_sums **sums, mtg_kmer_counts **kmer_counts,
                                               mtg_kmer_colors **kmer_colors, mtg_color_stats *color_stats, mtg_color_classes **classes) {
    if (!in) MTG_DIE("mtg_compact_unitigs_colored_classes_store: null argument");
    mtg_compact_unitigs_colored_classes(in->s->data.data(), in->s->off.data(), in->s->off.size() - 1, k, min_abundance, record_colors, n_colors, split,
                                        device_id, out, stats, abundance, sums, kmer_counts, kmer_colors, color_stats, classes);
}
// The rung is the highest one whose out-pointers are all there; a rung's inputs are read only where it is reached.
void mtg_compact_unitigs_cleaned(const char *data, const uint64_t *offsets, uint64_t n, uint64_t k, uint64_t min_abundance,
                                 const uint8_t *record_colors, uint64_t n_colors, int split, const mtg_cleaning_params *params, int device_id,
                                 mtg_unitigs **out, mtg_compaction *stats, mtg_abundance *abundance, mtg_abundance_sums **sums,
                                 mtg_kmer_counts **kmer_counts, mtg_kmer_colors **kmer_colors, mtg_color_stats *color_stats,
                                 mtg_color_classes **classes, mtg_cleaning *cleaning) {
    const char *const who = "mtg_compact_unitigs_cleaned";
    const CompactRung rung = !sums ? PLAIN : !kmer_counts ? COUNTED : (!kmer_colors || !color_stats) ? COUNTED_KMERS : !classes ? COLORED : CLASSES;
    if (rung < COUNTED && min_abundance != 1) MTG_DIE("%s: min_abundance %llu needs the sums' out-pointer", who, (unsigned long long)min_abundance);
    if (rung < CLASSES && split != 0) MTG_DIE("%s: split needs the classes' out-pointer", who);
    compact_call(who, rung, {data, offsets, n, k, device_id, min_abundance, record_colors, n_colors, split, params},
                 {out, stats, abundance, sums, kmer_counts, kmer_colors, color_stats, classes, cleaning});
}
void mtg_compact_unitigs_cleaned_store(const mtg_unitigs *in, uint64_t k, uint64_t min_abundance, const uint8_t *record_colors,
                                       uint64_t n_colors, int split, const mtg_cleaning_params *params, int device_id, mtg_unitigs **out,
                                       mtg_compaction *stats, mtg_abundance *abundance, mtg_abundance_sums **sums,
                                       mtg_kmer_counts **kmer_counts, mtg_kmer_colors **kmer_colors, mtg_color_stats *color_stats,
                                       mtg_color_classes **classes, mtg_cleaning *cleaning) {
    if (!in) MTG_DIE("mtg_compact_unitigs_cleaned_store: null argument");
    mtg_compact_unitigs_cleaned(in->s->data.data(), in->s->off.data(), in->s->off.size() - 1, k, min_abundance, record_colors, n_colors, split, params,
                                device_id, out, stats, abundance, sums, kmer_counts, kmer_colors, color_stats, classes, cleaning);
}
void mtg_last_clean_times(double out[2]) {
    out[0] = g_last_clean[0];
    out[1] = g_last_clean[1];
}
void mtg_compact_unitigs_simplified(const char *data, const uint64_t *offsets, uint64_t n, uint64_t k, uint64_t min_abundance,
                                    const uint8_t *record_colors, uint64_t n_colors, int split, const mtg_cleaning_params *params,
                                    const mtg_bubble_params *bubble_params, int device_id, mtg_unitigs **out, mtg_compaction *stats,
                                    mtg_abundance *abundance, mtg_abundance_sums **sums, mtg_kmer_counts **kmer_counts,
                                    mtg_kmer_colors **kmer_colors, mtg_color_stats *color_stats, mtg_color_classes **classes,
                                    mtg_cleaning *cleaning, mtg_bubbles *bubbles) {
    const char *const who = "mtg_compact_unitigs_simplified";
    const CompactRung rung = !sums ? PLAIN : !kmer_counts ? COUNTED : (!kmer_colors || !color_stats) ? COUNTED_KMERS : !classes ? COLORED : CLASSES;
    if (rung < COUNTED && min_abundance != 1) MTG_DIE("%s: min_abundance %llu needs the sums' out-pointer", who, (unsigned long long)min_abundance);
    if (rung < CLASSES && split != 0) MTG_DIE("%s: split needs the classes' out-pointer", who);
    if (rung >= COUNTED && bubble_params && bubbles && bubble_params->max_arm_kmers && !abundance)
        MTG_DIE("%s: popping bubbles compares abundances and needs the abundance and sums out-pointers", who);
    compact_call(who, rung, {data, offsets, n, k, device_id, min_abundance, record_colors, n_colors, split, params, bubble_params},
                 {out, stats, abundance, sums, kmer_counts, kmer_colors, color_stats, classes, cleaning, bubbles});
}
void mtg_compact_unitigs_simplified_store(const mtg_unitigs *in, uint64_t k, uint64_t min_abundance, const uint8_t *record_colors,
                                          uint64_t n_colors, int split, const mtg_cleaning_params *params,
                                          const mtg_bubble_params *bubble_params, int device_id, mtg_unitigs **out, mtg_compaction *stats,
                                          mtg_abundance *abundance, mtg_abundance_sums **sums, mtg_kmer_counts **kmer_counts,
                                          mtg_kmer_colors **kmer_colors, mtg_color_stats *color_stats, mtg_color_classes **classes,
                                          mtg_cleaning *cleaning, mtg_bubbles *bubbles) {
    if (!in) MTG_DIE("mtg_compact_unitigs_simplified_store: null argument");
    mtg_compact_unitigs_simplified(in->s->data.data(), in->s->off.data(), in->s->off.size() - 1, k, min_abundance, record_colors, n_colors, split, params,
                                   bubble_params, device_id, out, stats, abundance, sums, kmer_counts, kmer_colors, color_stats, classes, cleaning,
                                   bubbles);
}
void mtg_last_bubble_times(double out[1]) { out[0] = g_last_bubble; }
void mtg_compact_unitigs_selected(const char *data, const uint64_t *offsets, uint64_t n, uint64_t k, uint64_t min_abundance,
                                  const uint8_t *record_colors, uint64_t n_colors, int split, const mtg_cleaning_params *params,
                                  const mtg_bubble_params *bubble_params, const mtg_selection_params *selection_params,
                                  const char *filter_data, const uint64_t *filter_offsets, const uint8_t *filter_roles, uint64_t filter_n,
                                  int device_id, mtg_unitigs **out, mtg_compaction *stats, mtg_abundance *abundance, mtg_abundance_sums **sums,
                                  mtg_kmer_counts **kmer_counts, mtg_kmer_colors **kmer_colors, mtg_color_stats *color_stats,
                                  mtg_color_classes **classes, mtg_cleaning *cleaning, mtg_bubbles *bubbles, mtg_selection *selection) {
    const char *const who = "mtg_compact_unitigs_selected";
    const CompactRung rung = !sums ? PLAIN : !kmer_counts ? COUNTED : (!kmer_colors || !color_stats) ? COUNTED_KMERS : !classes ? COLORED : CLASSES;
    if (rung < COUNTED && min_abundance != 1) MTG_DIE("%s: min_abundance %llu needs the sums' out-pointer", who, (unsigned long long)min_abundance);
    if (rung < CLASSES && split != 0) MTG_DIE("%s: split needs the classes' out-pointer", who);
    if (rung >= COUNTED && bubble_params && bubbles && bubble_params->max_arm_kmers && !abundance)
        MTG_DIE("%s: popping bubbles compares abundances and needs the abundance and sums out-pointers", who);
    CompactIn in{data, offsets, n, k, device_id, min_abundance, record_colors, n_colors, split, params, bubble_params, selection_params};
    in.filter_data = filter_data;
    in.filter_offsets = filter_offsets;
    in.filter_roles = filter_roles;
    in.filter_n = filter_n;
    compact_call(who, rung, in, {out, stats, abundance, sums, kmer_counts, kmer_colors, color_stats, classes, cleaning, bubbles, selection});
}
void mtg_compact_unitigs_selected_store(const mtg_unitigs *in, uint64_t k, uint64_t min_abundance, const uint8_t *record_colors,
                                        uint64_t n_colors, int split, const mtg_cleaning_params *params,
                                        const mtg_bubble_params *bubble_params, const mtg_selection_params *selection_params,
                                        const char *filter_data, const uint64_t *filter_offsets, const uint8_t *filter_roles,
                                        uint64_t filter_n, int device_id, mtg_unitigs **out, mtg_compaction *stats, mtg_abundance *abundance,
                                        mtg_abundance_sums **sums, mtg_kmer_counts **kmer_counts, mtg_kmer_colors **kmer_colors,
                                        mtg_color_stats *color_stats, mtg_color_classes **classes, mtg_cleaning *cleaning,
                                        mtg_bubbles *bubbles, mtg_selection *selection) {
    if (!in) MTG_DIE("mtg_compact_unitigs_selected_store: null argument");
    mtg_compact_unitigs_selected(in->s->data.data(), in->s->off.data(), in->s->off.size() - 1, k, min_abundance, record_colors, n_colors, split, params,
                                 bubble_params, selection_params, filter_data, filter_offsets, filter_roles, filter_n, device_id, out, stats, abundance,
                                 sums, kmer_counts, kmer_colors, color_stats, classes, cleaning, bubbles, selection);
}
void mtg_last_select_times(double out[2]) {
    out[0] = g_last_compact.filter_ms;
    out[1] = g_last_compact.select_ms;
}
// the vector behind one of the handles above (who: the entry point, for the message)
extern "C++" {
template <class Handle>
static const auto &vector_of(const Handle *h, const char *who) {
    if (!h) MTG_DIE("%s: null argument", who);
    return h->v;
}
}
uint64_t mtg_abundance_sums_count(const mtg_abundance_sums *sums) { return vector_of(sums, "mtg_abundance_sums_count").size(); }
const uint64_t *mtg_abundance_sums_array(const mtg_abundance_sums *sums) { return vector_of(sums, "mtg_abundance_sums_array").data(); }
void mtg_abundance_sums_free(mtg_abundance_sums *sums) { delete sums; }
uint64_t mtg_kmer_counts_count(const mtg_kmer_counts *counts) { return vector_of(counts, "mtg_kmer_counts_count").size(); }
const uint32_t *mtg_kmer_counts_array(const mtg_kmer_counts *counts) { return vector_of(counts, "mtg_kmer_counts_array").data(); }
void mtg_kmer_counts_free(mtg_kmer_counts *counts) { delete counts; }
uint64_t mtg_kmer_colors_count(const mtg_kmer_colors *colors) { return vector_of(colors, "mtg_kmer_colors_count").size(); }
const uint64_t *mtg_kmer_colors_array(const mtg_kmer_colors *colors) { return vector_of(colors, "mtg_kmer_colors_array").data(); }
void mtg_kmer_colors_free(mtg_kmer_colors *colors) { delete colors; }
// ---- monochromatic unitigs and colour classes ----
void mtg_color_classes_build(const uint64_t *kmer_colors, uint64_t n, const uint64_t *unitig_kmers, uint64_t n_unitigs, int device_id,
                             mtg_color_classes **classes) {
    if (!classes) MTG_DIE("mtg_color_classes_build: null argument");
    mtg_color_classes *cl = new mtg_color_classes();
    device_color_classes(kmer_colors, n, unitig_kmers, n_unitigs, device_id, &cl->c, &g_last_color_class);
    *classes = cl;
}
static const ColorClasses &classes_of(const mtg_color_classes *classes, const char *who) {
    if (!classes) MTG_DIE("%s: null argument", who);
    return classes->c;
}
uint64_t mtg_color_classes_count(const mtg_color_classes *classes) { return classes_of(classes, "mtg_color_classes_count").masks.size(); }
const uint64_t *mtg_color_classes_masks(const mtg_color_classes *classes) { return classes_of(classes, "mtg_color_classes_masks").masks.data(); }
const uint64_t *mtg_color_classes_kmers(const mtg_color_classes *classes) { return classes_of(classes, "mtg_color_classes_kmers").kmers.data(); }
const uint64_t *mtg_color_classes_runs(const mtg_color_classes *classes) { return classes_of(classes, "mtg_color_classes_runs").runs.data(); }
const uint64_t *mtg_color_classes_first(const mtg_color_classes *classes) { return classes_of(classes, "mtg_color_classes_first").first.data(); }
uint64_t mtg_color_classes_kmer_class_count(const mtg_color_classes *classes) {
    return classes_of(classes, "mtg_color_classes_kmer_class_count").kmer_class.size();
}
const uint32_t *mtg_color_classes_kmer_class(const mtg_color_classes *classes) {
    return classes_of(classes, "mtg_color_classes_kmer_class").kmer_class.data();
}
void mtg_color_classes_free(mtg_color_classes *classes) { delete classes; }
void mtg_last_color_class_times(double out[5]) {
    const ColorClassTimes &t = g_last_color_class;
    out[0] = t.heads_ms; out[1] = t.table_ms; out[2] = t.ids_ms; out[3] = t.counts_ms; out[4] = t.download_ms;
}
void mtg_color_class_limits(uint64_t out[3]) {
    for (int i = 0; i < 3; i++) out[i] = device_color_class_limit(i);
}
void mtg_last_compact_times(double out[12]) {
    const CompactTimes &t = g_last_compact;
    out[0] = t.upload_ms; out[1] = t.pack_ms; out[2] = t.insert_ms; out[3] = t.ids_ms; out[4] = t.nodes_ms; out[5] = t.rank_ms;
    out[6] = t.emit_ms; out[7] = t.download_ms; out[8] = t.total_ms; out[9] = (double)t.rounds; out[10] = (double)t.bytes;
    out[11] = (double)t.peak_arena_bytes;
}
void mtg_read_sequences_split(const char *path, mtg_unitigs **store_out, uint64_t *pieces_cut) {
    if (!path || !store_out) MTG_DIE("mtg_read_sequences_split: null argument");
    *store_out = new mtg_unitigs{read_fasta_records_split(path, pieces_cut)};
}
static thread_local FastqTimes g_last_fastq;
int mtg_read_fastq_split(const char *path, uint64_t min_base_quality, int device_id, mtg_unitigs **store_out, mtg_fastq_stats *stats, char *err,
                         uint64_t err_capacity) {
    if (!path || !store_out) MTG_DIE("mtg_read_fastq_split: null argument");
    UnitigStore *st = nullptr;
    const int status = device_read_fastq(path, min_base_quality, device_id, false, &st, nullptr, stats, &g_last_fastq, err, err_capacity);
    if (status == 0) *store_out = new mtg_unitigs{st};
    return status;
}
int mtg_read_fastq_named(const char *path, uint64_t min_base_quality, int device_id, mtg_unitigs **seqs_out, mtg_unitigs **names_out,
                         mtg_fastq_stats *stats, char *err, uint64_t err_capacity) {
    if (!path || !seqs_out || !names_out) MTG_DIE("mtg_read_fastq_named: null argument");
    UnitigStore *st = nullptr, *names = nullptr;
    const int status = device_read_fastq(path, min_base_quality, device_id, true, &st, &names, stats, &g_last_fastq, err, err_capacity);
    if (status == 0) {
        *seqs_out = new mtg_unitigs{st};
        *names_out = new mtg_unitigs{names};
    }
    return status;
}
int mtg_sequence_file_format(const char *path) {
    if (!path) MTG_DIE("mtg_sequence_file_format: null argument");
    return fq::format_of_file(path);
}
void mtg_last_fastq_times(double out[6]) {
    const FastqTimes &t = g_last_fastq;
    out[0] = t.read_ms; out[1] = t.upload_ms; out[2] = t.lines_ms; out[3] = t.pieces_ms; out[4] = t.download_ms; out[5] = t.total_ms;
}
uint64_t mtg_unitigs_count(const mtg_unitigs *u) { return u->s->off.size() - 1; }
const char *mtg_unitigs_data(const mtg_unitigs *u) { return u->s->data.data(); }
const uint64_t *mtg_unitigs_offsets(const mtg_unitigs *u) { return u->s->off.data(); }
void mtg_unitigs_select(const mtg_unitigs *u, const uint8_t *keep, mtg_unitigs **out) {
    if (!u || !out || (mtg_unitigs_count(u) && !keep)) MTG_DIE("mtg_unitigs_select: null argument");
    const UnitigStore &in = *u->s;
    const uint64_t n = in.off.size() - 1;
    uint64_t records = 0, bytes = 0;
    for (uint64_t i = 0; i < n; i++)
        if (keep[i]) { records++; bytes += in.off[i + 1] - in.off[i]; }
    UnitigStore *st = new UnitigStore();
    st->data.reserve(bytes);
    st->off.reserve(records + 1);
    st->off.push_back(0);
    for (uint64_t i = 0; i < n; i++)
        if (keep[i]) {
            st->data.append(in.data, in.off[i], in.off[i + 1] - in.off[i]);
            st->off.push_back(st->data.size());
        }
    *out = new mtg_unitigs{st};
}
void mtg_unitigs_free(mtg_unitigs *u) {
    if (!u) return;
    delete u->s;
    delete u;
}
uint64_t mtg_write_tigs_text_file_device(const mtg_graph *g, const mtg_walks *tigs, uint64_t k, const mtg_unitigs *unitigs, int gfa,
                                         const char *gfa_header, const char *path, int compression_level, int device_id) {
    if (!g || !tigs || !unitigs || !path) MTG_DIE("mtg_write_tigs_text_file_device: null argument");
    char *buf = nullptr;
    // (tigs a finish on the same GPU left in HBM are spelled from there: no download, no upload)
    const ResidentTigs *res = tigs->resident_on(device_id);
    const uint64_t n = res ? device_write_walks_text(g->g, 0, nullptr, nullptr, k, unitigs->s->data.data(), unitigs->s->off.data(), gfa != 0, gfa_header, device_id, &buf,
                                                     &g_last_spell_kernel_ms, &g_last_spell_bytes, res)
                       : device_count() > device_id && device_id >= 0
                           ? device_write_walks_text(g->g, tigs->host().limits.size(), tigs->host().limits.data(), tigs->host().edges.data(), k, unitigs->s->data.data(),
                                                     unitigs->s->off.data(), gfa != 0, gfa_header, device_id, &buf, &g_last_spell_kernel_ms, &g_last_spell_bytes)
                           : write_walks_text(g->g, tigs->host().limits.size(), tigs->host().limits.data(), tigs->host().edges.data(), k,
                                              unitigs->s->data.data(), unitigs->s->off.data(), gfa != 0, gfa_header, &buf);
    write_file(path, buf, n, compression_level);
    std::free(buf);
    return n;
}
uint64_t mtg_write_tigs_fasta_file(const mtg_graph *g, const mtg_walks *tigs, uint64_t k, const mtg_unitigs *unitigs,
                                   const char *path, int compression_level) {
    return mtg_write_tigs_text_file_device(g, tigs, k, unitigs, 0, nullptr, path, compression_level, 0);
}
uint64_t mtg_write_tigs_gfa_file(const mtg_graph *g, const mtg_walks *tigs, uint64_t k, const mtg_unitigs *unitigs,
                                 const char *header, const char *path, int compression_level) {
    return mtg_write_tigs_text_file_device(g, tigs, k, unitigs, 1, header, path, compression_level, 0);
}

// ---- optimal matchtigs around the external matcher (matchtigs/mod.rs:150-940) ----
struct mtg_matching {
    MatchingInstance *m;
};
mtg_matching *mtg_matching_instance(const mtg_graph *g, const mtg_config *cfg) {
    check_config(cfg, "mtg_matching_instance");
    if (!g || !g->g.built) MTG_DIE("mtg_matching_instance: graph is not built");
    const uint64_t k = cfg->k;
    double t0 = now_s();
    mtg_device *dev = mtg_device_create(g, k, cfg->device_ids[0]);
    log_info("Collecting nodes with missing incoming or outgoing edges");
    const uint64_t S = mtg_classify(dev, nullptr);
    std::vector<uint32_t> out_nodes(S);
    std::vector<int32_t> mult(g->g.node_count());
    mtg_classify_download(dev, nullptr, out_nodes.data(), mult.data(), nullptr);
    log_info("Found %llu nodes with missing outgoing edges", (unsigned long long)S);
    log_info("Computing shortest paths between nodes with missing outgoing and nodes with missing incoming edges");
    std::vector<uint64_t> cand_start, pool;
    std::vector<uint32_t> cand_count;
    device_candidates_to_host(dev->d, nullptr, cand_start, cand_count, pool);
    mtg_device_free(dev);
    double t1 = now_s();
    MatchingInstance *m = build_matching_instance(g->g, k, S, out_nodes.data(), mult.data(), cand_start.data(), cand_count.data(), pool.data());
    log_info("Took %.6fs for computing paths and getting edges, of this %.6fs are from dijkstra", now_s() - t0, t1 - t0);
    log_info("Found %llu nodes and %zu edges", (unsigned long long)m->transformed_node_count, m->edge_n2.size());
    log_info("Matching problem contains %llu edges that originate from %llu mirror biedges", (unsigned long long)m->mirror_expanded_biedges,
             (unsigned long long)m->mirror_biedges);
    log_info("Found %llu relevant WCCs", (unsigned long long)m->wcc_amount);
    return new mtg_matching{m};
}
mtg_matching *mtg_matching_instance_from_lists(const mtg_graph *g, uint64_t k, uint64_t n_sources, const uint32_t *out_nodes,
                                               const int32_t *multiplicity, const uint64_t *cand_start, const uint32_t *cand_count,
                                               const uint64_t *pool) {
    if (!g || !g->g.built) MTG_DIE("mtg_matching_instance_from_lists: graph is not built");
    if (k < 1) MTG_DIE("mtg_matching_instance_from_lists: k must be >= 1");
    if (!multiplicity || (n_sources && (!out_nodes || !cand_start || !cand_count))) MTG_DIE("mtg_matching_instance_from_lists: null argument");
    return new mtg_matching{build_matching_instance(g->g, k, n_sources, out_nodes, multiplicity, cand_start, cand_count, pool)};
}
void mtg_matching_get_stats(const mtg_matching *m, mtg_matching_stats *out) {
    if (!m || !out) MTG_DIE("mtg_matching_get_stats: null argument");
    out->transformed_node_count = m->m->transformed_node_count;
    out->edge_count = m->m->edge_n2.size();
    out->wcc_amount = m->m->wcc_amount;
    out->matching_node_count = m->m->matching_node_count;
    out->matching_edge_count = m->m->matching_edge_count;
    out->mirror_biedges = m->m->mirror_biedges;
    out->mirror_expanded_biedges = m->m->mirror_expanded_biedges;
}
uint64_t mtg_matching_write(const mtg_matching *m, const char *path) {
    if (!m || !path) MTG_DIE("mtg_matching_write: null argument");
    log_info("Outputting matching problem to \"%s\"", path);
    return write_matching_instance(*m->m, path);
}
uint64_t mtg_matching_read_solution(const mtg_matching *m, const char *solution_path, mtg_pair **pairs_out) {
    if (!m || !solution_path || !pairs_out) MTG_DIE("mtg_matching_read_solution: null argument");
    std::vector<Pair> p = read_matching_solution(*m->m, solution_path);
    mtg_pair *out = (mtg_pair *)std::malloc(std::max<size_t>(p.size(), 1) * sizeof(mtg_pair));
    if (!out) MTG_DIE("out of memory");
    if (!p.empty()) std::memcpy(out, p.data(), p.size() * sizeof(mtg_pair));
    *pairs_out = out;
    return p.size();
}
void mtg_matching_free(mtg_matching *m) {
    if (!m) return;
    delete m->m;
    delete m;
}
mtg_walks *mtg_finish_matchtigs_cfg(mtg_graph *g, const mtg_pair *pairs, uint64_t n_pairs, const mtg_config *cfg) {
    check_config(cfg, "mtg_finish_matchtigs_cfg");
    if (!g || !g->g.built) MTG_DIE("mtg_finish_matchtigs_cfg: graph is not built");
    const uint64_t k = cfg->k;
    uint64_t bidirected = 0;
    for (uint64_t i = 0; i < n_pairs; i++) bidirected += pairs[i].out_node == g->g.mirror[pairs[i].in_node] ? 2 : 0;
    const uint64_t dummy_edge_id = insert_pair_edges(g->g, reinterpret_cast<const Pair *>(pairs), n_pairs);  // :797-808
    log_info("Inserted %llu matched edges", (unsigned long long)(2 * n_pairs));
    if (bidirected) log_info("Inserted %llu bidirected loops", (unsigned long long)bidirected);
    log_info("Making graph Eulerian by completing unmatched nodes");
    make_eulerian(g->g, dummy_edge_id, k);  // :831
    if (!is_eulerian(g->g)) MTG_DIE("Failed to make the graph Eulerian. (matchtigs/mod.rs:849)");
    log_info("Finding Eulerian bicycle");
    Walks cycles = euler_cycles_by_mode(g->g, *cfg);
    log_info("Found %zu Eulerian bicycles", cycles.limits.size());
    uint64_t begin = 0;
    for (uint64_t c = 0; c < cycles.limits.size(); c++) {  // :870-886
        uint64_t longest = 0;
        for (uint64_t i = begin; i < cycles.limits[c]; i++)
            if (g->g.is_dummy(cycles.edges[i])) longest = std::max<uint64_t>(longest, g->g.weight(cycles.edges[i]));
        if (longest > 0 && longest < k) MTG_DIE("Eulerian bicycle contains at least one dummy edge, but no breaking edge (matchtigs/mod.rs:883)");
        begin = cycles.limits[c];
    }
    mtg_walks *tigs = new mtg_walks{cut_cycles(g->g, cycles, k)};
    log_info("Found %zu matchtigs", (size_t)tigs->count());
    return tigs;
}
mtg_walks *mtg_compute_matchtigs_cfg(mtg_graph *g, const mtg_config *cfg) {
    check_config(cfg, "mtg_compute_matchtigs_cfg");
    if (!cfg->matching_file_prefix) MTG_DIE("mtg_compute_matchtigs_cfg: matching_file_prefix is null");
    if (!cfg->matcher_path) MTG_DIE("mtg_compute_matchtigs_cfg: matcher_path is null");
    mtg_matching *m = mtg_matching_instance(g, cfg);
    const std::string instance_path = std::string(cfg->matching_file_prefix) + ".minimalperfectmatching";  // :592-593
    const std::string solution_path = instance_path + ".solution";                                          // :722
    mtg_matching_write(m, instance_path.c_str());
    if (m->m->transformed_node_count != 0) {  // :724-741
        log_info("Running matcher at \"%s\"", cfg->matcher_path);
        const char *argv[] = {cfg->matcher_path, "-e", instance_path.c_str(), "-w", solution_path.c_str(), nullptr};
        pid_t pid = 0;
        const int rc = posix_spawnp(&pid, cfg->matcher_path, nullptr, nullptr, const_cast<char *const *>(argv), environ);  // searches PATH like Command::new (matchtigs/mod.rs:727)
        if (rc != 0) MTG_DIE("cannot start the matcher %s: %s", cfg->matcher_path, std::strerror(rc));
        int status = 0;
        while (waitpid(pid, &status, 0) < 0)
            if (errno != EINTR) MTG_DIE("waitpid on the matcher failed: %s", std::strerror(errno));
        if (!WIFEXITED(status) || WEXITSTATUS(status) != 0) MTG_DIE("Matcher was unsuccessful: wait status %d (matchtigs/mod.rs:735)", status);
    } else {
        log_info("Nothing to match, generating empty output file");  // :742-746
        FILE *f = std::fopen(solution_path.c_str(), "w");
        if (!f) MTG_DIE("cannot create %s", solution_path.c_str());
        std::fputs("0 0\n", f);
        std::fclose(f);
    }
    log_info("Applying matcher result to graph");
    mtg_pair *pairs = nullptr;
    const uint64_t n_pairs = mtg_matching_read_solution(m, solution_path.c_str(), &pairs);
    mtg_matching_free(m);
    mtg_walks *tigs = mtg_finish_matchtigs_cfg(g, pairs, n_pairs, cfg);
    std::free(pairs);
    return tigs;
}

static mtg_walks *compute_tigs_cfg_body(mtg_graph *g, uint64_t tig_algorithm, const mtg_config *cfg);
mtg_walks *mtg_compute_tigs_cfg(mtg_graph *g, uint64_t tig_algorithm, const mtg_config *cfg) {
    mtg_walks *w = compute_tigs_cfg_body(g, tig_algorithm, cfg);
    // what the graph's constructor reserved ahead on its default GPU is given back if this call ran elsewhere
    if (tig_algorithm >= 3) device_drop_foreign_reservation(cfg->device_ids, cfg->n_devices);
    return w;
}
static mtg_walks *compute_tigs_cfg_body(mtg_graph *g, uint64_t tig_algorithm, const mtg_config *cfg) {
    check_config(cfg, "mtg_compute_tigs_cfg");
    if (!g || !g->g.built) MTG_DIE("mtg_compute_tigs: graph is not built");
    for (double &p : g_phase) p = 0;
    g_last_perf = mtg_dijkstra_performance_data{};
    const uint64_t k = cfg->k;
    switch (tig_algorithm) {
        case 1: {  // clib.rs:351-361: one walk per forward unitig edge
            mtg_walks *w = new mtg_walks();
            for (uint64_t e = 0; e < g->g.edge_count(); e += 2) {
                w->w.edges.push_back((uint32_t)e);
                w->w.limits.push_back(w->w.edges.size());
            }
            return w;
        }
        case 3:
            return mtg_compute_eulertigs_cfg(g, cfg);
        case 5: {
            double t0 = now_s();
            // one resident copy of the graph per configured GPU (replicas + source sharding), built concurrently
            const int n_dev = cfg->n_devices;
            std::vector<mtg_device *> devs((size_t)n_dev, nullptr);
            {
                std::vector<std::thread> th;
                // (searched once: no goal-directed lower bounds -- their precompute costs several times what it saves one search)
                for (int i = 1; i < n_dev; i++) th.emplace_back([&, i]() { devs[(size_t)i] = mtg_device_create_opts(g, k, cfg->device_ids[i], MTG_DEVICE_NO_LOWER_BOUNDS); });
                devs[0] = mtg_device_create_opts(g, k, cfg->device_ids[0], MTG_DEVICE_NO_LOWER_BOUNDS);
                for (auto &t : th) t.join();
            }
            mtg_device *dev = devs[0];
            if (cfg->performance_data_type != MTG_PERFORMANCE_DATA_COMPLETE)  // (the counters are a second search)
                for (mtg_device *x : devs) device_set_single_use(x->d);
            double t1 = now_s();
            g_phase[0] = t1 - t0;
            log_info("Collecting nodes with missing incoming or outgoing edges");
            uint64_t S = 0;
            {
                std::vector<std::thread> th;
                for (int i = 1; i < n_dev; i++) th.emplace_back([&, i]() { (void)mtg_classify(devs[(size_t)i], nullptr); });
                S = mtg_classify(dev, nullptr);
                for (auto &t : th) t.join();
            }
            double t2 = now_s();
            g_phase[1] = t2 - t1;
            log_info("Found %llu nodes with missing outgoing edges", (unsigned long long)S);
            // SSSP candidates (sharded over the devices) and the claim loop both run on the GPU; only the matched pairs come back
            // ... and stay in the HBM of the first GPU when the finish runs there too (the default)
            const bool resident = use_device_finish(g->g, nullptr, 0, *cfg) && device_id_of(dev->d) == cfg->device_ids[0];
            mtg_pair *pairs = nullptr;
            uint64_t n_pairs = 0;
            {
                std::vector<Device *> dd((size_t)n_dev);
                for (int i = 0; i < n_dev; i++) dd[(size_t)i] = devs[(size_t)i]->d;
                double gather_ms = 0;
                n_pairs = device_pairs_multi(dd.data(), n_dev, resident ? nullptr : &pairs, nullptr, &gather_ms);
                g_last_gather_ms = gather_ms;
            }
            double t3 = now_s();
            {   // [2] SSSP stage (+ gather over the devices), [4] claim replay, [3] pair download (0 when the pairs stay in HBM)
                double w[3];
                device_last_pairs_wall_s(dev->d, w);
                g_phase[4] = w[1];
                g_phase[3] = w[2];
                g_phase[2] = std::max(0.0, (t3 - t2) - w[1] - w[2]);
            }
            for (int i = 1; i < n_dev; i++) mtg_device_free(devs[(size_t)i]);
            if (cfg->performance_data_type == MTG_PERFORMANCE_DATA_COMPLETE) {  // greedytigs/mod.rs:647-673
                device_performance_data(dev->d, nullptr, &g_last_perf);
                const mtg_dijkstra_performance_data &p = g_last_perf;
                if (p.iterations)
                    log_info("Dijkstras had a factor of %.3f unnecessary heap elements", (double)p.unnecessary_heap_elements / (double)p.iterations);
                log_info("Dijktras had a maximum maximum heap size of %llu", (unsigned long long)p.max_max_heap_size);
                log_info("Dijktras had a maximum maximum distance array size of %llu", (unsigned long long)p.max_max_distance_array_size);
                if (p.dijkstras) {
                    log_info("Dijktras had an average maximum heap size of %.0f", (double)p.sum_max_heap_size / (double)p.dijkstras);
                    log_info("Dijktras had an average maximum heap size of %.0f", (double)p.sum_max_distance_array_size / (double)p.dijkstras);  // sic, :669-671
                }
            }
            mtg_pair *d_pairs = resident ? device_take_pairs(dev->d, nullptr) : nullptr;  // (ours now: the device graph can go before the finish)
            mtg_device_free(dev);
            log_info("Found %llu shortest paths", (unsigned long long)n_pairs);
            mtg_walks *tigs;
            if (resident) {
                tigs = finish_on_device(g->g, nullptr, n_pairs, *cfg, d_pairs);
                log_info("Found %zu greedytigs", tig_count(tigs));
                device_free_array(cfg->device_ids[0], d_pairs);
                if (std::getenv("MTG_DEBUG")) {
                    uint64_t a[4];
                    device_arena_stats(cfg->device_ids[0], a);
                    std::fprintf(stderr, "[mtg] device arena: %.2f GB in chunks (%llu taken from the driver so far), peak of live arrays %.2f GB, estimate for this graph %.2f GB\n",
                                 a[0] / 1e9, (unsigned long long)a[3], a[2] / 1e9, device_call_bytes_estimate(g->g.node_count(), g->g.n_original_edges, k) / 1e9);
                }
            } else {
                tigs = mtg_finish_greedytigs_cfg(g, pairs, n_pairs, cfg);
                std::free(pairs);
            }
            return tigs;
        }
        case 2:
            MTG_DIE("tig algorithm 2 (pathtigs) is outside the scope of the MI355X engine (SURVEY.md 2, row 11)");
        case 4:  // clib.rs:362-376: needs the external matcher the configuration names
            return mtg_compute_matchtigs_cfg(g, cfg);
        default:
            MTG_DIE("Unknown tigs algorithm identifier %llu", (unsigned long long)tig_algorithm);  // clib.rs:390
    }
    return nullptr;
}

// The whole path into a caller's clib.rs output arrays (sized as clib.rs:332-348: 2 E, 2 E and E entries for E original edges):
// what matchtigs_compute_tigs does after it has built its configuration. With a finish on the GPU the tigs never exist as walks on
// the host: the host threads that empty the download ring write the flattened form (clib.rs:393-407) straight into the caller's
// arrays, whose pages a helper thread touches while the GPU stages run.
uint64_t mtg_compute_tigs_clib(mtg_graph *g, uint64_t tig_algorithm, const mtg_config *cfg, int64_t *tigs_edge_out, uint64_t *tigs_insert_out,
                               uint64_t *tigs_out_limits) {
    check_config(cfg, "mtg_compute_tigs_clib");
    if (!g || !g->g.built) MTG_DIE("mtg_compute_tigs_clib: graph is not built");
    if (!tigs_edge_out || !tigs_insert_out || !tigs_out_limits) MTG_DIE("mtg_compute_tigs_clib: null output array");
    TigSink sink;
    sink.edge_out = tigs_edge_out;
    sink.insert_out = tigs_insert_out;
    sink.limits_out = tigs_out_limits;
    const uint64_t E0 = g->g.n_original_edges;
    std::thread toucher;
    if ((tig_algorithm == 5 || tig_algorithm == 3) && E0 >= (1u << 22) && use_device_finish(g->g, nullptr, 0, *cfg)) {
        // fresh output arrays cost a page fault per 4 KB when they are first written: a few threads take those faults now, beside the
        // device-graph build and the search (tigs hold one edge per unitig and a few matched dummies; a tig per four unitigs is plenty)
        const uint64_t n_e = E0 / 2 + E0 / 8, n_l = E0 / 4;
        // (advice only: where the caller's arrays are anonymous memory and the system hands out huge pages on request, a fault brings 2 MB)
        for (auto r : {std::make_pair((char *)tigs_edge_out, n_e * 8), std::make_pair((char *)tigs_insert_out, n_e * 8), std::make_pair((char *)tigs_out_limits, n_l * 8)}) {
            const uintptr_t lo = ((uintptr_t)r.first + (2u << 20) - 1) & ~(uintptr_t)((2u << 20) - 1), hi = ((uintptr_t)r.first + r.second) & ~(uintptr_t)((2u << 20) - 1);
            if (hi > lo) (void)madvise((void *)lo, hi - lo, MADV_HUGEPAGE);
        }
        toucher = std::thread([=]() {
            const double t_touch = now_s();
            parallel_ranges((n_e * 8 + 4095) / 4096, [&](uint64_t lo, uint64_t hi) {
                for (uint64_t pg = lo; pg < hi; pg++) {
                    *((volatile char *)tigs_edge_out + pg * 4096) = 0;
                    *((volatile char *)tigs_insert_out + pg * 4096) = 0;
                }
            }, 6);
            parallel_ranges((n_l * 8 + 4095) / 4096, [&](uint64_t lo, uint64_t hi) {
                for (uint64_t pg = lo; pg < hi; pg++) *((volatile char *)tigs_out_limits + pg * 4096) = 0;
            }, 6);
            if (std::getenv("MTG_DEBUG")) std::fprintf(stderr, "[mtg] output arrays touched (%.2f GB) %.1f ms after the call began\n", (2 * n_e + n_l) * 8 / 1e9, (now_s() - t_touch) * 1e3);
        });
    }
    if (toucher.joinable()) sink.pretoucher = &toucher;  // joined by the finish before its first write into the arrays
    g_clib_sink = &sink;
    g_clib_sink_used = false;
    mtg_walks *tigs = mtg_compute_tigs_cfg(g, tig_algorithm, cfg);
    g_clib_sink = nullptr;
    if (toucher.joinable()) toucher.join();
    const uint64_t n = g_clib_sink_used ? sink.n_tigs : flatten_clib(g->g, tigs->host(), tigs_edge_out, tigs_insert_out, tigs_out_limits);
    delete tigs;
    return n;
}

mtg_walks *mtg_compute_tigs(mtg_graph *g, uint64_t tig_algorithm, uint64_t k, int device_id) {
    mtg_config cfg;
    mtg_config_init(&cfg, 1, k);
    cfg.device_ids[0] = device_id;
    return mtg_compute_tigs_cfg(g, tig_algorithm, &cfg);
}

void mtg_last_performance_data(mtg_dijkstra_performance_data *out) {
    if (out) *out = g_last_perf;
}

void mtg_last_phase_seconds(double out[8]) {
    for (int i = 0; i < 8; i++) out[i] = g_phase[i];
}

// ------------------------------------------------------------------------------------------------
// matchtigs.h: the reference's C-ABI (src/clib.rs)
// ------------------------------------------------------------------------------------------------
void matchtigs_initialise(void) {  // clib.rs:87-92
    g_log_initialised = true;
    log_info("Logging initialised successfully");
}

MatchtigsData *matchtigs_initialise_graph(size_t unitig_amount) {  // clib.rs:94-102
    HostGraph *h = builder_new(unitig_amount);
    MatchtigsData *d = new MatchtigsData{mtg_graph{std::move(*h)}};
    delete h;
    return d;
}

void matchtigs_merge_nodes(MatchtigsData *data, size_t unitig_a, bool strand_a, size_t unitig_b, bool strand_b) {  // clib.rs:135-170
    if (!data) MTG_DIE("matchtigs_merge_nodes: matchtigs_data is null");
    builder_merge(&data->graph.g, unitig_a, strand_a, unitig_b, strand_b);
}

void matchtigs_build_graph(MatchtigsData *data, const size_t *unitig_weights) {  // clib.rs:180-259
    if (!data) MTG_DIE("matchtigs_build_graph: matchtigs_data is null");
    static_assert(sizeof(size_t) == sizeof(uint64_t), "64-bit only");
    double t0 = now_s();
    builder_build(&data->graph.g, reinterpret_cast<const uint64_t *>(unitig_weights));
    log_info("Took %.6fs to build the tig graph", now_s() - t0);
}

size_t matchtigs_compute_tigs(MatchtigsData *data, size_t tig_algorithm, size_t threads, size_t k,
                              const char *matching_file_prefix, const char *matcher_path, ptrdiff_t *tigs_edge_out,
                              size_t *tigs_insert_out, size_t *tigs_out_limits) {  // clib.rs:280-410
    if (!data) MTG_DIE("matchtigs_compute_tigs: matchtigs_data is null");
    log_info("Computing tigs for k = %zu and %zu threads", k, threads);
    log_info("Graph has %llu nodes and %llu edges", (unsigned long long)data->graph.g.node_count(),
             (unsigned long long)data->graph.g.edge_count());
    if (!matching_file_prefix) MTG_DIE("assertion failed: !matching_file_prefix.is_null() (clib.rs:300)");
    if (!matcher_path) MTG_DIE("assertion failed: !matcher_path.is_null() (clib.rs:316)");
    if (!tigs_edge_out) MTG_DIE("assertion failed: !tigs_edge_out.is_null() (clib.rs:333)");
    if (!tigs_insert_out) MTG_DIE("assertion failed: !tigs_insert_out.is_null() (clib.rs:339)");
    if (!tigs_out_limits) MTG_DIE("assertion failed: !tigs_out_limits.is_null() (clib.rs:345)");
    static_assert(sizeof(ptrdiff_t) == sizeof(int64_t), "64-bit only");
    mtg_config cfg;  // clib.rs:378-389: staged None, factor 1, StdBinaryHeap, EpochNodeWeightArray, performance data None
    mtg_config_init(&cfg, threads, k);
    cfg.resource_limit_factor = 1;
    cfg.node_weight_array_type = MTG_NODE_WEIGHT_EPOCH_ARRAY;
    cfg.matching_file_prefix = matching_file_prefix;  // clib.rs:362-376
    cfg.matcher_path = matcher_path;
    const uint64_t n = mtg_compute_tigs_clib(&data->graph, tig_algorithm, &cfg, reinterpret_cast<int64_t *>(tigs_edge_out),
                                             reinterpret_cast<uint64_t *>(tigs_insert_out), reinterpret_cast<uint64_t *>(tigs_out_limits));
    free_graph_object(data, data->graph.g);  // Box::from_raw at clib.rs:291: the handle is consumed
    return n;
}

}  // extern "C"
