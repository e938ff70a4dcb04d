// tig_index_file_device.hpp -- the sparse minimizer index written to a file and read back (the format: tig_index_file.hpp)
//
// Included by tig_index_device.hip at its end, behind the TigIndex struct: the sections of a file ARE the struct's device
// arrays, byte for byte, so a save is digest -> download -> write and a load is read -> upload -> digest -> validate, with no rebuild.
//
// array_digest_kernel: the digest of tig_index_file.hpp over a device array. The sum of mix(w_i ^ (i + 1) STEP) is commutative, so
// the schedule cannot change it: a thread strides over PAIRS of words (one 16-byte load each), a wave folds its lanes with
// __shfl_down, lane 0 of every wave leaves its partial in LDS (EB / 64 words, nothing else), thread 0 adds them and leaves by ONE
// 64-bit atomicAdd per workgroup (spectrum_kernel's rule). The odd last word and the zero-padded tail bytes are read by
// thread 0 of block 0. The host XORs the word count in.
//
// index_validate_kernel: a loaded file is untrusted input that becomes pointer arithmetic in the probes. What they assume of the
// arrays (the list is DESIGN.md 35's) is checked here, independent of the digests, by a grid-stride loop over the longest array;
// every read is bounded by the array's own count, which the host checks have tied to the allocation. Errors leave through one flags
// word (stretch_measure_kernel's way), one bit per section.
//
// A refused file is an error of the input: device_tig_index_load returns null and says why, with every allocation returned.
#pragma once

#include <fcntl.h>
#include <unistd.h>

#include <cerrno>
#include <memory>
#include <string>

#include "tig_index_file.hpp"

namespace mtg {
namespace tfd {

constexpr unsigned DIGEST_BLOCKS = 2048;  // 8 per compute unit: enough loads in flight for a streaming read

static __global__ __launch_bounds__(hu::EB) void array_digest_kernel(const unsigned char *bytes, uint64_t n_bytes, unsigned long long *out) {
    __shared__ unsigned long long wave_sum[hu::EB / 64];
    const uint64_t full = n_bytes / 8, pairs = full / 2;
    const ulonglong2 *v = reinterpret_cast<const ulonglong2 *>(bytes);  // (an arena range: 4096-byte aligned)
    unsigned long long sum = 0;
    for (uint64_t i = hu::gid(), step = (uint64_t)gridDim.x * blockDim.x; i < pairs; i += step) {
        const ulonglong2 w = v[i];
        sum += tf::mix(w.x ^ ((2 * i + 1) * tf::DIGEST_STEP)) + tf::mix(w.y ^ ((2 * i + 2) * tf::DIGEST_STEP));
    }
    if (hu::gid() == 0) {
        if (full & 1) sum += tf::mix(reinterpret_cast<const unsigned long long *>(bytes)[full - 1] ^ (full * tf::DIGEST_STEP));
        if (n_bytes & 7) {
            unsigned long long w = 0;
            for (uint64_t b = full * 8; b < n_bytes; b++) w |= (unsigned long long)bytes[b] << (8 * (b - full * 8));
            sum += tf::mix(w ^ ((full + 1) * tf::DIGEST_STEP));
        }
    }
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long all = 0;
        for (int w = 0; w < hu::EB / 64; w++) all += wave_sum[w];
        if (all) atomicAdd(out, all);
    }
}

// *out (zeroed before on st) += the digest's sum over the array; nothing is launched for an empty one
inline void digest_launch(const void *d, uint64_t n_bytes, unsigned long long *out, hipStream_t st) {
    if (!n_bytes) return;
    const unsigned grid = std::min<unsigned>(DIGEST_BLOCKS, std::max<unsigned>(1, hu::grid_for(n_bytes / 16)));
    array_digest_kernel<<<grid, hu::EB, 0, st>>>(static_cast<const unsigned char *>(d), n_bytes, out);
    HIP_CHECK(hipGetLastError());
}

enum : unsigned {  // the validator's flags: bit s = section s of tf::Section
    BAD_OFF = 1u << tf::OFF, BAD_DIR = 1u << tf::DIR, BAD_ENTRIES = 1u << tf::ENTRIES, BAD_TABLE = 1u << tf::TABLE,
    BAD_HEAVY_WHERE = 1u << tf::HEAVY_WHERE, BAD_WIN_OFF = 1u << tf::WIN_OFF, BAD_W_START = 1u << tf::W_START,
    BAD_C_DENSE = 1u << tf::C_DENSE, BAD_C_START = 1u << tf::C_START, BAD_C_VALUE = 1u << tf::C_VALUE
};
inline const char *validate_check(int section) {
    switch (section) {
    case tf::OFF: return "the record offsets start at 0, do not decrease and end at `characters`";
    case tf::DIR: return "the bucket starts begin at 0, do not decrease, keep at most bucket_limit anchors each (none in a heavy bucket) and end at `anchors`";
    case tf::ENTRIES: return "every anchor's m bases lie inside one record of the text and the anchors of a bucket ascend by position";
    case tf::TABLE: return "every occupied slot names k bases inside one record of the text (k >= 32) or a code of 2 k bits";
    case tf::HEAVY_WHERE: return "every occupied slot's window start has its k bases inside one record of the text";
    case tf::WIN_OFF: return "the windows before every record start at 0, grow by each record's windows and end at `occurrences`";
    case tf::W_START: case tf::C_START: return "the run starts begin at 0, ascend and stay below `windows`";
    default: return "no mask has a bit from n_colors on";
    }
}

struct ValidateArgs {
    const unsigned long long *off, *win_off, *dir, *entries, *table, *heavy_where;  // win_off, table, heavy_where: null if absent
    uint64_t records, characters, occurrences, k, m, buckets, anchors, bucket_limit, table_slots;
    const unsigned long long *w_start, *c_start, *c_value;  // null unless the payload is kept as runs
    const unsigned char *c_dense;                           // null unless the masks are dense
    uint64_t w_runs, c_runs, c_width, n_colors;
    unsigned int *flags;
    unsigned long long *sums;  // [2], zeroed: the windows of all records; the heavy buckets
};

// [p, p + len) lies inside the record that holds p (off need not be sound: the search stays inside [0, records])
__device__ __forceinline__ bool inside_one_record(const ValidateArgs &a, uint64_t p, uint64_t len) {
    if (!a.records || p >= a.characters) return false;
    const uint64_t r = kr::record_of(a.off, a.records, p);
    return a.off[r] <= p && a.off[r + 1] <= a.characters && p + len <= a.off[r + 1];
}
__device__ __forceinline__ bool run_start_ok(const unsigned long long *start, uint64_t runs, uint64_t windows, uint64_t i) {
    const uint64_t s = start[i];
    return (i ? true : s == 0) && s < windows && (i + 1 < runs ? start[i + 1] > s : true);
}

static __global__ __launch_bounds__(hu::EB) void index_validate_kernel(ValidateArgs a, uint64_t n) {
    constexpr unsigned long long HEAVY_BIT = 1ull << 63;
    unsigned int bad = 0;
    unsigned long long windows = 0, heavy = 0;
    for (uint64_t i = hu::gid(), step = (uint64_t)gridDim.x * blockDim.x; i < n; i += step) {
        if (i <= a.records) {
            const uint64_t o = a.off[i];
            if ((i == 0 && o != 0) || (i == a.records && o != a.characters)) bad |= BAD_OFF;
            if (a.win_off && ((i == 0 && a.win_off[0] != 0) || (i == a.records && a.win_off[i] != a.occurrences))) bad |= BAD_WIN_OFF;
            if (i < a.records) {
                const uint64_t next = a.off[i + 1];
                if (next < o || next > a.characters) bad |= BAD_OFF;
                else {
                    const uint64_t w = next - o >= a.k ? next - o - a.k + 1 : 0;
                    windows += w;
                    if (a.win_off && a.win_off[i + 1] - a.win_off[i] != w) bad |= BAD_WIN_OFF;
                }
            }
        }
        if (i <= a.buckets) {
            const unsigned long long d = a.dir[i];
            if ((i == 0 && (d & ~HEAVY_BIT) != 0) || (i == a.buckets && d != a.anchors)) bad |= BAD_DIR;
            if (i < a.buckets) {
                const uint64_t lo = d & ~HEAVY_BIT, hi = a.dir[i + 1] & ~HEAVY_BIT;
                if (d & HEAVY_BIT) heavy++;
                if (hi < lo || hi > a.anchors || hi - lo > a.bucket_limit || ((d & HEAVY_BIT) && hi != lo)) bad |= BAD_DIR;
                else
                    for (uint64_t j = lo + 1; j < hi; j++)  // (at most bucket_limit)
                        if ((a.entries[j - 1] & tf::POS_LIMIT) >= (a.entries[j] & tf::POS_LIMIT)) bad |= BAD_ENTRIES;
            }
        }
        if (i < a.anchors && !inside_one_record(a, a.entries[i] & tf::POS_LIMIT, a.m)) bad |= BAD_ENTRIES;
        if (i < a.table_slots) {
            const unsigned long long cur = a.table[i];
            if (cur != ~0ull && (a.k >= 32 ? !inside_one_record(a, cur & tf::POS_LIMIT, a.k) : (cur >> (2 * a.k)) != 0)) bad |= BAD_TABLE;
            if (a.heavy_where) {
                const unsigned long long t = a.heavy_where[i];
                if (cur == ~0ull ? t != ~0ull : !inside_one_record(a, t, a.k)) bad |= BAD_HEAVY_WHERE;
            }
        }
        if (a.w_start && i < a.w_runs && !run_start_ok(a.w_start, a.w_runs, a.occurrences, i)) bad |= BAD_W_START;
        if (a.c_start && i < a.c_runs) {
            if (!run_start_ok(a.c_start, a.c_runs, a.occurrences, i)) bad |= BAD_C_START;
            if (a.n_colors < 64 && (a.c_value[i] >> a.n_colors)) bad |= BAD_C_VALUE;
        }
        if (a.c_dense && i < a.occurrences && a.n_colors < 64) {
            unsigned long long mask;
            switch (a.c_width) {
            case 1: mask = a.c_dense[i]; break;
            case 2: mask = reinterpret_cast<const uint16_t *>(a.c_dense)[i]; break;
            case 4: mask = reinterpret_cast<const uint32_t *>(a.c_dense)[i]; break;
            default: mask = reinterpret_cast<const unsigned long long *>(a.c_dense)[i]; break;
            }
            if (mask >> a.n_colors) bad |= BAD_C_DENSE;
        }
    }
    if (bad) atomicOr(a.flags, bad);
    if (windows) atomicAdd(&a.sums[0], windows);
    if (heavy) atomicAdd(&a.sums[1], heavy);
}

// the device array of every section: where it is and how many bytes of it the file holds
struct Sections {
    const void *d[tf::N_SECTIONS];
    uint64_t bytes[tf::N_SECTIONS];
};
inline Sections sections_of(const TigIndex *ix, const tf::Header &h) {
    Sections s;
    const void *d[tf::N_SECTIONS] = {ix->packed.get(), ix->off.get(), ix->dir.get(), ix->entries.get(), ix->table.get(), ix->heavy_where.get(), ix->win_off.get(),
                                     ix->weights.dense.get(), ix->weights.start.get(), ix->weights.value.get(),
                                     ix->colors.dense.get(), ix->colors.start.get(), ix->colors.value.get()};
    for (int i = 0; i < tf::N_SECTIONS; i++) {
        s.bytes[i] = h.sec[i].elem_size * h.sec[i].count;
        s.d[i] = s.bytes[i] ? d[i] : nullptr;
    }
    return s;
}

// the digests of all sections, computed on the device over the arrays as they lie there; returns the kernels' time
inline double digest_sections(const Sections &s, uint64_t out[tf::N_SECTIONS], hipStream_t st) {
    hu::DeviceArray<unsigned long long> d_sum(tf::N_SECTIONS);
    unsigned long long sums[tf::N_SECTIONS];
    PhaseEvents<2> ev;
    HIP_CHECK(hipMemsetAsync(d_sum, 0, sizeof sums, st));
    ev.mark(0, st);
    for (int i = 0; i < tf::N_SECTIONS; i++) digest_launch(s.d[i], s.bytes[i], d_sum + i, st);
    ev.mark(1, st);
    HIP_CHECK(hipMemcpyAsync(sums, d_sum, sizeof sums, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    for (int i = 0; i < tf::N_SECTIONS; i++) out[i] = ((s.bytes[i] + 7) / 8) ^ sums[i];
    return ev.ms(0, 1);
}

struct Fd {  // a file descriptor that closes itself
    int fd = -1;
    ~Fd() { if (fd >= 0) ::close(fd); }
};
inline bool write_all(int fd, const void *p, size_t n) {
    const char *c = static_cast<const char *>(p);
    while (n) {
        const ssize_t w = ::write(fd, c, n);
        if (w < 0 && errno == EINTR) continue;
        if (w <= 0) return false;
        c += w;
        n -= (size_t)w;
    }
    return true;
}
inline bool read_all(int fd, void *p, size_t n, uint64_t at) {
    char *c = static_cast<char *>(p);
    while (n) {
        const ssize_t r = ::pread(fd, c, n, (off_t)at);
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) return false;
        c += r;
        at += (uint64_t)r;
        n -= (size_t)r;
    }
    return true;
}
inline bool write_zeros(int fd, uint64_t n) {
    static const char zeros[tf::ALIGN] = {};
    for (; n; n -= std::min<uint64_t>(n, tf::ALIGN))
        if (!write_all(fd, zeros, std::min<uint64_t>(n, tf::ALIGN))) return false;
    return true;
}

}  // namespace tfd

// The index as a file at `path` (written beside it as path + ".tmp" and renamed at the end). The arrays leave slice by slice through
// the pinned ring of the sliced transfers: the host holds RING_SLOTS slices, never the index. false: err says why (an error of the
// output file; the index is untouched).
bool device_tig_index_save(const TigIndex *ix, const char *path, const char *meta, uint64_t meta_len, TigIndexFileTimes *times, std::string &err) {
    on_device(ix->device_id);
    hipStream_t st = nullptr;
    if (times) times->save_digest_ms = times->save_download_ms = times->save_write_ms = 0;
    tf::Header h{};
    mtg_tig_payload_info pl;
    device_tig_index_payload_info(ix, &pl);
    tf::header_fill(h, ix->info, ix->shift, ix->locating, pl, meta_len);
    const tfd::Sections s = tfd::sections_of(ix, h);
    uint64_t digests[tf::N_SECTIONS];
    const double digest_ms = tfd::digest_sections(s, digests, st);  // before the download: of what lies in device memory
    for (int i = 0; i < tf::N_SECTIONS; i++) h.sec[i].digest = digests[i];
    h.meta_digest = tf::digest_bytes(meta, meta_len);
    tf::header_seal(h);

    const std::string tmp = std::string(path) + ".tmp";
    double download_ms = 0, write_ms = 0;
    bool ok = false;
    {
        tfd::Fd f;
        f.fd = ::open(tmp.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
        if (f.fd < 0) { err = tmp + ": cannot create: " + std::strerror(errno); return false; }
        auto t0 = std::chrono::steady_clock::now();
        uint64_t at = tf::HEADER_BYTES + 8 + meta_len;
        ok = tfd::write_all(f.fd, &h, sizeof h) && tfd::write_all(f.fd, &meta_len, 8) && tfd::write_all(f.fd, meta, meta_len);
        write_ms += ms_since(t0);
        hu::TransferRing &ring = hu::transfer_ring(ix->device_id);
        std::lock_guard<std::mutex> lock(ring.m);
        ring.ready();
        for (int i = 0; i < tf::N_SECTIONS && ok; i++) {
            t0 = std::chrono::steady_clock::now();
            ok = tfd::write_zeros(f.fd, h.sec[i].offset - at);
            write_ms += ms_since(t0);
            at = h.sec[i].offset + s.bytes[i];
            // slice j + 1 crosses while slice j is written
            const uint64_t n_slices = (s.bytes[i] + hu::RING_SLICE - 1) / hu::RING_SLICE;
            for (uint64_t j = 0; j <= n_slices && ok; j++) {
                t0 = std::chrono::steady_clock::now();
                if (j < n_slices) {
                    const uint64_t o = j * hu::RING_SLICE, n = std::min<uint64_t>(hu::RING_SLICE, s.bytes[i] - o);
                    HIP_CHECK(hipMemcpyAsync(ring.slot[j % 2], static_cast<const char *>(s.d[i]) + o, n, hipMemcpyDeviceToHost, st));
                    HIP_CHECK(hipEventRecord(ring.ev[j % 2], st));
                }
                if (j > 0) HIP_CHECK(hipEventSynchronize(ring.ev[(j - 1) % 2]));
                download_ms += ms_since(t0);
                if (j > 0) {
                    t0 = std::chrono::steady_clock::now();
                    const uint64_t o = (j - 1) * hu::RING_SLICE, n = std::min<uint64_t>(hu::RING_SLICE, s.bytes[i] - o);
                    ok = tfd::write_all(f.fd, ring.slot[(j - 1) % 2], n);
                    write_ms += ms_since(t0);
                }
            }
        }
        HIP_CHECK(hipStreamSynchronize(st));
        const auto t1 = std::chrono::steady_clock::now();
        ok = ok && tfd::write_zeros(f.fd, h.file_len - at) && ::fsync(f.fd) == 0;
        write_ms += ms_since(t1);
        if (!ok) err = tmp + ": cannot write: " + std::strerror(errno);
    }
    if (ok && ::rename(tmp.c_str(), path) != 0) {
        err = std::string(path) + ": cannot rename " + tmp + " to it: " + std::strerror(errno);
        ok = false;
    }
    if (!ok) (void)::unlink(tmp.c_str());
    if (times) { times->save_digest_ms = digest_ms; times->save_download_ms = download_ms; times->save_write_ms = write_ms; }
    return ok;
}

// The index of the file at `path`, or null: err names the path, the section and the check, and every allocation has gone back. The
// header and the metadata have passed the host checks (tf::header_read) before anything is allocated; then the sections are uploaded
// through the pinned ring, digested on the device, and validated there.
TigIndex *device_tig_index_load(const char *path, int device_id, std::string &meta, TigIndexFileTimes *times, std::string &err) {
    if (times) times->load_read_ms = times->load_upload_ms = times->load_digest_ms = times->load_validate_ms = 0;
    tf::Header h;
    if (!tf::header_read(path, h, meta, err)) return nullptr;
    if (device_id < 0 || device_count() <= device_id) MTG_DIE("no HIP device %d for the tig index (there is no CPU path)", device_id);
    on_device(device_id);
    hipStream_t st = nullptr;
    struct Free { void operator()(TigIndex *ix) const { device_tig_index_free(ix); } };
    std::unique_ptr<TigIndex, Free> ix(new TigIndex());
    mtg_tig_payload_info pl;
    tf::header_info(h, &ix->info, &pl);
    ix->device_id = device_id;
    ix->shift = (uint32_t)h.shift;
    ix->locating = h.locating != 0;
    ix->n_colors = h.n_colors;
    ix->weights.info = pl.weights;
    ix->colors.info = pl.colors;
    const mtg_tig_index_info &info = ix->info;
    // the allocations of the builders, element for element (what the file does not hold of them is never read)
    ix->packed.alloc((info.characters + 15) / 16 + 2);
    ix->off.alloc(info.records + 1);
    ix->dir.alloc(info.buckets + 1);
    ix->entries.alloc(std::max<uint64_t>(info.anchors, 1));
    if (info.table_slots) ix->table.alloc(info.table_slots);
    if (info.table_slots && ix->locating) ix->heavy_where.alloc(info.table_slots);
    if (pl.win_offset_bytes) ix->win_off.alloc(info.records + 1);
    if (pl.weights.layout == tp::LAYOUT_DENSE) ix->weights.dense.alloc(std::max<uint64_t>(pl.weights.device_bytes, 1));
    if (pl.weights.layout == tp::LAYOUT_RUNS) { ix->weights.start.alloc(std::max<uint64_t>(pl.weights.runs, 1)); ix->weights.value.alloc(std::max<uint64_t>(pl.weights.runs, 1)); }
    if (pl.colors.layout == tp::LAYOUT_DENSE) ix->colors.dense.alloc(std::max<uint64_t>(pl.colors.device_bytes, 1));
    if (pl.colors.layout == tp::LAYOUT_RUNS) { ix->colors.start.alloc(std::max<uint64_t>(pl.colors.runs, 1)); ix->colors.value.alloc(std::max<uint64_t>(pl.colors.runs, 1)); }
    const tfd::Sections s = tfd::sections_of(ix.get(), h);

    double read_ms = 0, upload_ms = 0;
    {
        tfd::Fd f;
        f.fd = ::open(path, O_RDONLY);
        if (f.fd < 0) { err = std::string(path) + ": cannot open: " + std::strerror(errno); return nullptr; }
        hu::TransferRing &ring = hu::transfer_ring(device_id);
        std::lock_guard<std::mutex> lock(ring.m);
        ring.ready();
        uint64_t sent = 0;  // slices queued so far, over all sections: slice `sent` uses slot sent % 2
        for (int i = 0; i < tf::N_SECTIONS; i++)
            for (uint64_t o = 0; o < s.bytes[i]; o += hu::RING_SLICE, sent++) {
                const uint64_t n = std::min<uint64_t>(hu::RING_SLICE, s.bytes[i] - o);
                auto t0 = std::chrono::steady_clock::now();
                if (sent >= 2) HIP_CHECK(hipEventSynchronize(ring.ev[sent % 2]));  // the slot's last slice has crossed
                upload_ms += ms_since(t0);
                t0 = std::chrono::steady_clock::now();
                const bool got = tfd::read_all(f.fd, ring.slot[sent % 2], n, h.sec[i].offset + o);
                read_ms += ms_since(t0);
                if (!got) {
                    HIP_CHECK(hipStreamSynchronize(st));
                    err = std::string(path) + ": section " + tf::section_name(i) + ": cannot read it: " + std::strerror(errno);
                    return nullptr;
                }
                t0 = std::chrono::steady_clock::now();
                HIP_CHECK(hipMemcpyAsync(static_cast<char *>(const_cast<void *>(s.d[i])) + o, ring.slot[sent % 2], n, hipMemcpyHostToDevice, st));
                HIP_CHECK(hipEventRecord(ring.ev[sent % 2], st));
                upload_ms += ms_since(t0);
            }
        const auto t0 = std::chrono::steady_clock::now();
        HIP_CHECK(hipStreamSynchronize(st));
        upload_ms += ms_since(t0);
    }
    if (times) { times->load_read_ms = read_ms; times->load_upload_ms = upload_ms; }

    // the digests, after the upload: of what lies in device memory
    uint64_t digests[tf::N_SECTIONS];
    const double digest_ms = tfd::digest_sections(s, digests, st);
    if (times) times->load_digest_ms = digest_ms;
    for (int i = 0; i < tf::N_SECTIONS; i++)
        if (digests[i] != h.sec[i].digest) {
            err = std::string(path) + ": section " + tf::section_name(i) + ": digest: the bytes on the device do not give the digest in the header";
            return nullptr;
        }

    // the invariants the probes rely on
    tfd::ValidateArgs a{};
    a.off = ix->off; a.win_off = ix->win_off; a.dir = ix->dir; a.entries = ix->entries; a.table = ix->table; a.heavy_where = ix->heavy_where;
    a.records = info.records; a.characters = info.characters; a.occurrences = info.occurrences; a.k = info.k; a.m = info.m;
    a.buckets = info.buckets; a.anchors = info.anchors; a.bucket_limit = info.bucket_limit; a.table_slots = info.table_slots;
    a.w_start = ix->weights.start; a.w_runs = pl.weights.layout == tp::LAYOUT_RUNS ? pl.weights.runs : 0;
    a.c_start = ix->colors.start; a.c_value = ix->colors.value; a.c_runs = pl.colors.layout == tp::LAYOUT_RUNS ? pl.colors.runs : 0;
    a.c_dense = ix->colors.dense; a.c_width = pl.colors.width; a.n_colors = h.n_colors;
    hu::DeviceArray<unsigned long long> d_out(3);  // the flags word, then the two sums
    unsigned long long out[3];
    a.flags = reinterpret_cast<unsigned int *>(d_out.get());
    a.sums = d_out + 1;
    uint64_t n = std::max({info.records + 1, info.buckets + 1, info.anchors, info.table_slots, a.w_runs, a.c_runs, a.c_dense ? info.occurrences : 0});
    PhaseEvents<2> ev;
    HIP_CHECK(hipMemsetAsync(d_out, 0, sizeof out, st));
    ev.mark(0, st);
    tfd::index_validate_kernel<<<std::min<unsigned>(tfd::DIGEST_BLOCKS, hu::grid_for(n)), hu::EB, 0, st>>>(a, n);
    HIP_CHECK(hipGetLastError());
    ev.mark(1, st);
    HIP_CHECK(hipMemcpyAsync(out, d_out, sizeof out, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (times) times->load_validate_ms = ev.ms(0, 1);
    const unsigned flags = (unsigned)out[0];
    int bad = -1;
    for (int i = 0; i < tf::N_SECTIONS && bad < 0; i++)
        if (flags >> i & 1) bad = i;
    if (bad < 0 && out[1] != info.occurrences) bad = tf::OFF;
    if (bad < 0 && out[2] != info.heavy_buckets) bad = tf::DIR;
    if (bad >= 0) {
        err = std::string(path) + ": section " + tf::section_name(bad) + ": validation: it does not hold that " + tfd::validate_check(bad);
        if (!flags && bad == tf::OFF) err += " (the records' windows do not add up to `occurrences`)";
        if (!flags && bad == tf::DIR) err += " (the heavy buckets are not as many as `heavy_buckets`)";
        return nullptr;
    }
    return ix.release();
}

}  // namespace mtg
