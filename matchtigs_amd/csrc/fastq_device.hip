// fastq_device.hip -- FASTQ reads read on the GPU (`--seq-in reads.fq`, `--query-fa reads.fq`, `--min-base-quality`).
//
// CONTRACT. The inflated text is a sequence of lines ended by "\n"; one "\r" before the "\n" belongs to the line end; a missing final
// "\n" is supplied and empty lines at the end are dropped (fastq_text.hpp, on the host), but when three lines remain of the last
// record, the end of the text is its quality line, of length 0. Record r is lines 4r .. 4r+3: line 4r begins
// with `@`, line 4r+2 with `+`, lines 4r+1 (bases) and 4r+3 (qualities) have the same length, every quality byte lies in '!' .. '~'.
// The kind of a line is its index mod 4 and nothing else. A file that breaks a rule is refused with the smallest (record, rule) that
// does -- an atomicMin over 64-bit words, so the answer does not depend on the launch geometry --, never with an abort.
// Base j of a record is GOOD when it is one of ACGTacgt and qual[j] - 33 >= Q. Split mode: the pieces are the maximal runs of good
// bases, upper-cased, in file order (read_fasta_records_split's rule with "not good" for "not ACGT"; pieces_cut counts the runs of
// bases that are not good). Named mode: the records whole, characters as they are, a base with qual[j] - 33 < Q replaced by `N`.
//
// KERNELS. The text is cut into tiles of FQ_TILE bytes, one block per tile, 16 bytes (one load) per thread.
//   lines   fq_newline_count_kernel -> scan over the tiles -> fq_line_start_kernel: line_start[i] = offset of line i (u64), [L] = T
//   check   fq_check_kernel, one thread per record: the structural rules (and the record lengths of the named mode)
//   pieces  fq_count_kernel: per tile the good bases and the piece starts, the quality rule, the statistics (block sums, one atomic
//           per counter and block) -> two scans over the tiles -> fq_emit_kernel: the same classification again, ranks inside the
//           tile by a block scan, the tile's bases staged in LDS and written as one contiguous range, the piece offsets beside them.
//           Every output position comes from a scan: the store is in file order and two runs give the same bytes.
//   named   fq_emit_named_kernel: out[record offset + j] per base, record offsets from a scan of the lengths; fq_header_start_kernel
//           compacts line_start[4r] for the host, which slices the names out of its copy of the text.
// All arrays come from the device arena and go back before the call returns. There is no CPU path.
#include <chrono>
#include <string>
#include <vector>

#include "device.hpp"
#include "fastq_text.hpp"
#include "hip_util.hpp"
#include "pack_device.hpp"

namespace mtg {
namespace {

constexpr int FQ_BYTES = 16;                   // text bytes per thread
constexpr int FQ_TILE = hu::EB * FQ_BYTES;     // text bytes per block

struct FqArgs {
    const unsigned char *text;      // [T], readable up to the next multiple of FQ_TILE (zeros)
    uint64_t T;
    const unsigned long long *ls;   // line_start [L + 1]
    uint64_t R;                     // complete records: L / 4
    uint32_t qmin;                  // 33 + Q: the smallest quality byte of a good base
};

__device__ __forceinline__ void load16(const unsigned char *text, uint64_t p0, unsigned char (&b)[FQ_BYTES]) {
    const uint4 v = *reinterpret_cast<const uint4 *>(text + p0);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < FQ_BYTES; i++) b[i] = (unsigned char)((w[i >> 2] >> (8 * (i & 3))) & 0xFFu);
}
__device__ __forceinline__ uint32_t newlines16(const unsigned char (&b)[FQ_BYTES]) {
    uint32_t n = 0;
#pragma unroll
    for (int i = 0; i < FQ_BYTES; i++) n += b[i] == '\n';
    return n;
}
// where the content of line l ends: before its "\n" and before one "\r" in front of that
__device__ __forceinline__ uint64_t content_end(const FqArgs &a, uint64_t l) {
    const uint64_t s = a.ls[l];
    uint64_t e = a.ls[l + 1] - 1;
    if (e > s && a.text[e - 1] == '\r') e--;
    return e;
}

static __global__ __launch_bounds__(hu::EB) void fq_newline_count_kernel(const unsigned char *text, uint32_t *tile_nl) {
    unsigned char b[FQ_BYTES];
    load16(text, (uint64_t)blockIdx.x * FQ_TILE + (uint64_t)threadIdx.x * FQ_BYTES, b);
    uint32_t total;
    hu::block_exclusive_scan<uint32_t>(newlines16(b), &total);
    if (threadIdx.x == 0) tile_nl[blockIdx.x] = total;
}

// tile_line[t] = the lines that end before tile t
static __global__ __launch_bounds__(hu::EB) void fq_line_start_kernel(const unsigned char *text, const unsigned long long *tile_line,
                                                                     unsigned long long *ls) {
    const uint64_t p0 = (uint64_t)blockIdx.x * FQ_TILE + (uint64_t)threadIdx.x * FQ_BYTES;
    unsigned char b[FQ_BYTES];
    load16(text, p0, b);
    uint32_t total;
    uint64_t at = tile_line[blockIdx.x] + hu::block_exclusive_scan<uint32_t>(newlines16(b), &total) + 1;
    if (p0 == 0) ls[0] = 0;
#pragma unroll
    for (int i = 0; i < FQ_BYTES; i++)
        if (b[i] == '\n') ls[at++] = p0 + i + 1;
}

static __global__ __launch_bounds__(hu::EB) void fq_check_kernel(FqArgs a, uint32_t *reclen, unsigned long long *err) {
    const uint64_t r = hu::gid();
    if (r >= a.R) return;
    const uint64_t l = 4 * r;
    const uint64_t len1 = content_end(a, l + 1) - a.ls[l + 1], len3 = content_end(a, l + 3) - a.ls[l + 3];
    uint32_t reason = 0;
    if (a.text[a.ls[l]] != '@') reason = fq::BAD_HEADER;
    else if (a.text[a.ls[l + 2]] != '+') reason = fq::BAD_SEPARATOR;
    else if (len1 != len3) reason = fq::BAD_LENGTH;
    else if (len1 > 0xFFFFFFFFull) reason = fq::LINE_TOO_LONG;
    if (reason) atomicMin(err, (unsigned long long)r << 8 | reason);
    if (reclen) reclen[r] = (uint32_t)len1;
}

// Calls f(i, ch, record, j, q, acgt, good, prev_good) for every byte b[i] of the thread that is base j of a complete record, in text
// order: q its quality byte, prev_good whether base j - 1 of the same record is good (false at j = 0). `line` = the index of the
// line that holds byte p0. A record whose quality line is the shorter one (refused by fq_check_kernel) reads '~' past its end.
template <typename F>
__device__ __forceinline__ void for_each_base(const FqArgs &a, uint64_t p0, const unsigned char (&b)[FQ_BYTES], uint64_t line, F &&f) {
    bool have = false, seq = false, prev_good = false;
    uint64_t start = 0, end = 0, qstart = 0, qlen = 0;
#pragma unroll
    for (int i = 0; i < FQ_BYTES; i++) {
        const uint64_t p = p0 + i;
        if (p >= a.T) break;
        const unsigned char ch = b[i];
        if (!have) {  // the first byte of the thread or of a line
            have = true;
            prev_good = false;
            seq = (line & 3) == 1 && (line >> 2) < a.R;
            if (seq) {
                start = a.ls[line];
                end = content_end(a, line);
                qstart = a.ls[line + 2];
                qlen = content_end(a, line + 2) - qstart;
                if (p > start && p < end) {
                    const uint64_t j = p - 1 - start;
                    const unsigned char q = j < qlen ? a.text[qstart + j] : (unsigned char)'~';
                    prev_good = base_code(a.text[p - 1]) < 4 && q >= a.qmin;
                }
            }
        }
        if (seq && p < end) {
            const uint64_t j = p - start;
            const unsigned char q = j < qlen ? a.text[qstart + j] : (unsigned char)'~';
            const bool acgt = base_code(ch) < 4, good = acgt && q >= a.qmin;
            f(i, ch, line >> 2, j, q, acgt, good, prev_good);
            prev_good = good;
        }
        if (ch == '\n') {
            line++;
            have = false;
        }
    }
}

// stats: [0] bases, [1] bases outside ACGT, [2] ACGT bases masked by quality, [3] runs of bases that are not good
static __global__ __launch_bounds__(hu::EB) void fq_count_kernel(FqArgs a, const unsigned long long *tile_line, uint32_t *tile_good,
                                                                uint32_t *tile_start, unsigned long long *stats, unsigned long long *err) {
    const uint64_t p0 = (uint64_t)blockIdx.x * FQ_TILE + (uint64_t)threadIdx.x * FQ_BYTES;
    unsigned char b[FQ_BYTES];
    load16(a.text, p0, b);
    uint32_t total;
    const uint64_t line = tile_line[blockIdx.x] + hu::block_exclusive_scan<uint32_t>(newlines16(b), &total);
    uint32_t good_n = 0, start_n = 0, bases = 0, other = 0, masked = 0, cuts = 0;
    for_each_base(a, p0, b, line, [&](int, unsigned char, uint64_t rec, uint64_t j, unsigned char q, bool acgt, bool good, bool prev_good) {
        bases++;
        other += !acgt;
        masked += acgt && !good;
        good_n += good;
        start_n += good && !prev_good;
        cuts += !good && (j == 0 || prev_good);
        if (q < 33 || q > 126) atomicMin(err, (unsigned long long)rec << 8 | fq::BAD_QUALITY);
    });
    // (a tile holds at most FQ_TILE = 2^12 of anything: two counters share a word)
    uint32_t t_pieces, t_bases, t_quality;
    hu::block_exclusive_scan<uint32_t>(good_n | start_n << 16, &t_pieces);
    hu::block_exclusive_scan<uint32_t>(bases | other << 16, &t_bases);
    hu::block_exclusive_scan<uint32_t>(masked | cuts << 16, &t_quality);
    if (threadIdx.x == 0) {
        tile_good[blockIdx.x] = t_pieces & 0xFFFFu;
        tile_start[blockIdx.x] = t_pieces >> 16;
        if (t_bases & 0xFFFFu) atomicAdd(stats + 0, (unsigned long long)(t_bases & 0xFFFFu));
        if (t_bases >> 16) atomicAdd(stats + 1, (unsigned long long)(t_bases >> 16));
        if (t_quality & 0xFFFFu) atomicAdd(stats + 2, (unsigned long long)(t_quality & 0xFFFFu));
        if (t_quality >> 16) atomicAdd(stats + 3, (unsigned long long)(t_quality >> 16));
    }
}

// good_before[t] / start_before[t]: the good bases / piece starts in the tiles before t. out [good bases], piece_off [pieces] (the
// host appends the end).
static __global__ __launch_bounds__(hu::EB) void fq_emit_kernel(FqArgs a, const unsigned long long *tile_line, const unsigned long long *good_before,
                                                               const unsigned long long *start_before, char *out, unsigned long long *piece_off) {
    __shared__ char stage[FQ_TILE];
    const uint64_t p0 = (uint64_t)blockIdx.x * FQ_TILE + (uint64_t)threadIdx.x * FQ_BYTES;
    unsigned char b[FQ_BYTES];
    load16(a.text, p0, b);
    uint32_t total;
    const uint64_t line = tile_line[blockIdx.x] + hu::block_exclusive_scan<uint32_t>(newlines16(b), &total);
    uint32_t flags = 0;  // bit i: byte i is a good base; bit 16 + i: it starts a piece
    for_each_base(a, p0, b, line, [&](int i, unsigned char, uint64_t, uint64_t, unsigned char, bool, bool good, bool prev_good) {
        if (good) flags |= (prev_good ? 1u : 0x10001u) << i;
    });
    const uint32_t ex = hu::block_exclusive_scan<uint32_t>(__popc(flags & 0xFFFFu) | __popc(flags >> 16) << 16, &total);
    const uint64_t out0 = good_before[blockIdx.x];
    uint32_t at = ex & 0xFFFFu;
    uint64_t piece = start_before[blockIdx.x] + (ex >> 16);
#pragma unroll
    for (int i = 0; i < FQ_BYTES; i++) {
        if (!(flags >> i & 1u)) continue;
        if (flags >> (16 + i) & 1u) piece_off[piece++] = out0 + at;
        stage[at++] = (char)(b[i] & 0xDFu);  // (a letter: upper case)
    }
    __syncthreads();
    const uint32_t n = total & 0xFFFFu;
    for (uint32_t i = threadIdx.x; i < n; i += hu::EB) out[out0 + i] = stage[i];
}

// seq_off[r] = the bases of the records before r
static __global__ __launch_bounds__(hu::EB) void fq_emit_named_kernel(FqArgs a, const unsigned long long *tile_line, const unsigned long long *seq_off,
                                                                     char *out) {
    const uint64_t p0 = (uint64_t)blockIdx.x * FQ_TILE + (uint64_t)threadIdx.x * FQ_BYTES;
    unsigned char b[FQ_BYTES];
    load16(a.text, p0, b);
    uint32_t total;
    const uint64_t line = tile_line[blockIdx.x] + hu::block_exclusive_scan<uint32_t>(newlines16(b), &total);
    for_each_base(a, p0, b, line, [&](int, unsigned char ch, uint64_t rec, uint64_t j, unsigned char q, bool, bool, bool) {
        out[seq_off[rec] + j] = q < a.qmin ? 'N' : (char)ch;
    });
}

static __global__ void fq_header_start_kernel(const unsigned long long *ls, uint64_t R, unsigned long long *header_start) {
    const uint64_t r = hu::gid();
    if (r < R) header_start[r] = ls[4 * r];
}

// the arena ranges of one call: all of them go back when the call returns, whichever way
struct Ranges {
    std::vector<const void *> v;
    ~Ranges() { for (const void *p : v) hu::device_free(p); }
    template <typename T>
    T *take(uint64_t count) {
        T *p = nullptr;
        hu::device_malloc(&p, (count ? count : 1) * sizeof(T));
        v.push_back(p);
        return p;
    }
};

}  // namespace

int device_read_fastq(const char *path, uint64_t min_base_quality, int device_id, bool named, UnitigStore **seqs_out, UnitigStore **names_out,
                      mtg_fastq_stats *stats_out, FastqTimes *times, char *err, uint64_t err_capacity) {
    if (!path || !seqs_out || (named && !names_out)) MTG_DIE("mtg_read_fastq: null argument");
    if (min_base_quality > 93) MTG_DIE("mtg_read_fastq: min_base_quality must be in 0 .. 93");
    if (err && err_capacity) err[0] = 0;
    const auto t_total = std::chrono::steady_clock::now();
    FastqTimes t{};
    mtg_fastq_stats s{};
    s.tile_bytes = FQ_TILE;
    fq::Text text = fq::read_inflated(path);
    fq::normalise(text);
    t.read_ms = ms_since(t_total);
    uint64_t T = text.n_one_more;  // (with an empty line behind the text, until the line count says whether it completes a record)
    std::unique_ptr<UnitigStore> store(new UnitigStore()), names(new UnitigStore());
    store->off.push_back(0);
    names->off.push_back(0);
    auto finish = [&]() {
        t.total_ms = ms_since(t_total);
        if (stats_out) *stats_out = s;
        if (times) *times = t;
        *seqs_out = store.release();
        if (named) *names_out = names.release();
        return 0;
    };
    if (T == 0) return finish();
    if (device_id < 0 || device_count() <= device_id) MTG_DIE("no HIP device %d for the FASTQ reader (there is no CPU path)", device_id);
    HIP_CHECK(hipSetDevice(device_id));
    hipStream_t st = nullptr;

    // ---- upload ----
    auto t0 = std::chrono::steady_clock::now();
    uint64_t n_tiles = (T + FQ_TILE - 1) / FQ_TILE;
    const uint64_t padded = n_tiles * FQ_TILE;
    if (n_tiles >= (1ull << 31)) MTG_DIE("mtg_read_fastq: %llu bytes of text; the limit is 2^43", (unsigned long long)T);
    Ranges mem;
    ScalarBlock small(st);  // [0] the smallest (record, reason) of a broken rule, [2..5] the statistics of fq_count_kernel
    unsigned char *d_text = mem.take<unsigned char>(padded);
    if (padded > T) HIP_CHECK(hipMemsetAsync(d_text + T, 0, padded - T, st));
    hu::upload_sliced(d_text, text.data(), T, st, device_id);
    t.upload_ms = ms_since(t0);

    // ---- lines and the structural check ----
    PhaseEvents<3> ev;
    ev.mark(0, st);
    const uint64_t nb = hu::scan_blocks(n_tiles);
    uint32_t *d_tile_nl = mem.take<uint32_t>(n_tiles);
    unsigned long long *d_tile_line = mem.take<unsigned long long>(n_tiles);
    uint64_t *d_bsum = mem.take<uint64_t>(nb + 2);
    fq_newline_count_kernel<<<(unsigned)n_tiles, hu::EB, 0, st>>>(d_text, d_tile_nl);
    HIP_CHECK(hipGetLastError());
    hu::scan_u32<uint64_t>(st, d_tile_nl, n_tiles, reinterpret_cast<uint64_t *>(d_tile_line), d_bsum, d_bsum + nb + 1);
    uint64_t L = 0;
    HIP_CHECK(hipMemcpyAsync(&L, d_bsum + nb + 1, 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (T > text.n && L % 4 != 0) {  // the empty line behind the text completes no record: it goes the way of the other empty lines
        HIP_CHECK(hipMemsetAsync(d_text + text.n, 0, T - text.n, st));
        T = text.n;
        L -= 1;
        n_tiles = (T + FQ_TILE - 1) / FQ_TILE;
    }
    const uint64_t R = L / 4;
    unsigned long long *d_ls = mem.take<unsigned long long>(L + 1);
    fq_line_start_kernel<<<(unsigned)n_tiles, hu::EB, 0, st>>>(d_text, d_tile_line, d_ls);
    HIP_CHECK(hipGetLastError());
    FqArgs a{d_text, T, d_ls, R, (uint32_t)(33 + min_base_quality)};
    uint32_t *d_reclen = named ? mem.take<uint32_t>(R) : nullptr;
    if (R) fq_check_kernel<<<hu::grid_for(R), hu::EB, 0, st>>>(a, d_reclen, small.d);
    HIP_CHECK(hipGetLastError());
    ev.mark(1, st);

    // ---- pieces: count (with the quality rule) ----
    uint32_t *d_tile_good = mem.take<uint32_t>(n_tiles), *d_tile_start = mem.take<uint32_t>(n_tiles);
    fq_count_kernel<<<(unsigned)n_tiles, hu::EB, 0, st>>>(a, d_tile_line, d_tile_good, d_tile_start, small.d + 2, small.d);
    HIP_CHECK(hipGetLastError());
    small.read(st, "FASTQ reader");
    unsigned long long first_error = small.h[0];
    if (L % 4) first_error = std::min(first_error, fq::pack_error(R, fq::TRUNCATED));
    if (first_error != fq::NO_ERROR) {
        fq::format_error(path, first_error, L, err, err_capacity);
        return 1;
    }
    s.records = R;
    s.bases = small.h[2];
    s.non_acgt_bases = small.h[3];
    s.masked_bases = small.h[4];
    s.pieces_cut = small.h[5];

    char *d_out = nullptr;
    if (!named) {  // ---- scan, emit ----
        unsigned long long *d_good_before = mem.take<unsigned long long>(n_tiles), *d_start_before = mem.take<unsigned long long>(n_tiles);
        uint64_t *d_bsum2 = mem.take<uint64_t>(nb + 2);
        hu::scan_u32<uint64_t>(st, d_tile_good, n_tiles, reinterpret_cast<uint64_t *>(d_good_before), d_bsum, d_bsum + nb + 1);
        hu::scan_u32<uint64_t>(st, d_tile_start, n_tiles, reinterpret_cast<uint64_t *>(d_start_before), d_bsum2, d_bsum2 + nb + 1);
        HIP_CHECK(hipMemcpyAsync(&s.bases_kept, d_bsum + nb + 1, 8, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(&s.pieces, d_bsum2 + nb + 1, 8, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        d_out = mem.take<char>(s.bases_kept);
        unsigned long long *d_piece_off = mem.take<unsigned long long>(s.pieces);
        fq_emit_kernel<<<(unsigned)n_tiles, hu::EB, 0, st>>>(a, d_tile_line, d_good_before, d_start_before, d_out, d_piece_off);
        HIP_CHECK(hipGetLastError());
        ev.mark(2, st);
        HIP_CHECK(hipStreamSynchronize(st));
        t0 = std::chrono::steady_clock::now();
        store->data.resize(s.bases_kept);
        store->off.resize(s.pieces + 1);
        hu::download_sliced(&store->data[0], d_out, s.bases_kept, st, device_id);
        hu::download_sliced(store->off.data(), d_piece_off, s.pieces * 8, st, device_id);
        store->off[s.pieces] = s.bases_kept;
    } else {
        s.pieces = R;
        s.bases_kept = s.bases;
        const uint64_t nbr = hu::scan_blocks(R);
        unsigned long long *d_seq_off = mem.take<unsigned long long>(R), *d_header = mem.take<unsigned long long>(R);
        uint64_t *d_bsum2 = mem.take<uint64_t>(nbr + 2);
        hu::scan_u32<uint64_t>(st, d_reclen, R, reinterpret_cast<uint64_t *>(d_seq_off), d_bsum2, d_bsum2 + nbr + 1);
        d_out = mem.take<char>(s.bases);
        fq_emit_named_kernel<<<(unsigned)n_tiles, hu::EB, 0, st>>>(a, d_tile_line, d_seq_off, d_out);
        if (R) fq_header_start_kernel<<<hu::grid_for(R), hu::EB, 0, st>>>(d_ls, R, d_header);
        HIP_CHECK(hipGetLastError());
        ev.mark(2, st);
        HIP_CHECK(hipStreamSynchronize(st));
        t0 = std::chrono::steady_clock::now();
        std::vector<uint64_t> header(R);
        store->data.resize(s.bases);
        store->off.resize(R + 1);
        hu::download_sliced(&store->data[0], d_out, s.bases, st, device_id);
        hu::download_sliced(store->off.data(), d_seq_off, R * 8, st, device_id);
        hu::download_sliced(header.data(), d_header, R * 8, st, device_id);
        store->off[R] = s.bases;
        fq::slice_names(text.data(), T, header.data(), R, names->data, names->off);
    }
    t.download_ms = ms_since(t0);
    t.lines_ms = ev.ms(0, 1);
    t.pieces_ms = ev.ms(1, 2);
    return finish();
}

}  // namespace mtg
