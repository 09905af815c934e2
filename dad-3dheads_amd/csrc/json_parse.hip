// Reading JSON on the device: the large arrays of numbers of a document lifted into float64, the doubles json.load
// makes (dad_3dheads_benchmark/benchmark.py:177-180). The kernels index the document and validate candidate arrays; matching the
// brackets (a stable sort by depth) and choosing the arrays is list work the caller does between the entries (json_reader.py).
//
// The document is cut into tiles of DAD3D_JSON_PARSE_TILE_BYTES = 256 lanes x 16 consecutive bytes. Every scan over it is three
// launches -- per-tile totals, one workgroup that scans the totals, apply -- so no workgroup ever waits on another:
//   json_tile_quotes_kernel    unescaped quotes per tile (a quote behind an odd run of backslashes is escaped; the look back over
//                              the run only reads, crosses tiles, and ends at byte 0)
//   json_scan_tiles_kernel     exclusive scan of per-tile columns, the totals to the caller's counts
//   json_classify_kernel       string state from the quote parity in front of every byte -> one class byte per byte (the only per-byte
//                              scratch), and per tile: tokens, brackets, non-numeric bytes, depth change
//   json_compact_kernel        token and bracket lists in document order, each entry with the counts in front of it
//   json_check_arrays_kernel   one workgroup per candidate array: shape, separators and every token through the number routine
//   json_values_kernel         one lane per value of a lifted array: json_parse_number -> float64 bits + is_int
// Stores are plain vector stores; there are no atomics. The sums and scans over a workgroup are those of collectives.hpp.
#include "common.hpp"
#include "json_parse_number.hpp"
#include "text_tile.hpp"

namespace dad3d {
namespace {

constexpr int kLanes = kTextTile;
constexpr int kLaneBytes = kTextLaneBytes;
static_assert(kLanes * kLaneBytes == DAD3D_JSON_PARSE_TILE_BYTES, "a tile is one 16-byte chunk per lane");

enum : unsigned { kWs = 0, kNonNum = 1, kOpen = 2, kClose = 3, kComma = 4, kNum = 5, kNumStart = 6 };

__device__ inline void store_chunk(unsigned char* __restrict__ dst, long long base, int valid, const uint4& v) {
    if (valid == kLaneBytes) {
        *reinterpret_cast<uint4*>(dst + base) = v;
    } else {
#pragma unroll
        for (int k = 0; k < kLaneBytes; ++k)
            if (k < valid) dst[base + k] = (unsigned char)byte_of(v, k);
    }
}

// bit k: byte k of the chunk is a quote with an even run of backslashes in front of it
__device__ inline unsigned unescaped_quotes(const unsigned char* __restrict__ text, long long base, const uint4& v, int valid) {
    unsigned mask = 0;
#pragma unroll
    for (int k = 0; k < kLaneBytes; ++k) {
        if (k < valid && byte_of(v, k) == '"') {
            long long j = base + k - 1;
            while (j >= 0 && text[j] == '\\') --j;  // reads only; ends at byte 0
            if ((((base + k - 1) - j) & 1) == 0) mask |= 1u << k;
        }
    }
    return mask;
}

__global__ __launch_bounds__(kLanes) void json_tile_quotes_kernel(const unsigned char* __restrict__ text, long long n, int* __restrict__ tile_quotes) {
    __shared__ int red[kTextWaves];
    const long long base = (long long)blockIdx.x * DAD3D_JSON_PARSE_TILE_BYTES + threadIdx.x * kLaneBytes;
    int valid;
    const uint4 v = load_chunk(text, base, n, valid);
    const int total = block_sum<kTextWaves>((int)__popc(unescaped_quotes(text, base, v, valid)), red);
    if (threadIdx.x == 0) tile_quotes[blockIdx.x] = total;
}

// data [ncols][ntiles] -> exclusive scan of every column in place, its total to totals[col] (when given). One workgroup.
__global__ __launch_bounds__(kLanes) void json_scan_tiles_kernel(int* __restrict__ data, int ntiles, int ncols, int* __restrict__ totals) {
    __shared__ int red[kTextWaves];
    for (int col = 0; col < ncols; ++col) {
        int* column = data + (size_t)col * ntiles;
        int carry = 0;
        for (int start = 0; start < ntiles; start += kLanes) {
            const int i = start + (int)threadIdx.x;
            const int v = i < ntiles ? column[i] : 0;
            int total;
            const int before = block_exclusive_scan<kTextWaves>(v, red, total);
            if (i < ntiles) column[i] = carry + before;
            carry += total;
        }
        if (totals && threadIdx.x == 0) totals[col] = carry;
    }
}

__global__ __launch_bounds__(kLanes) void json_classify_kernel(const unsigned char* __restrict__ text, long long n, int ntiles,
                                                               const int* __restrict__ tile_quotes, unsigned char* __restrict__ cls,
                                                               int* __restrict__ tile_totals) {
    __shared__ int red[kTextWaves];
    const long long base = (long long)blockIdx.x * DAD3D_JSON_PARSE_TILE_BYTES + threadIdx.x * kLaneBytes;
    int valid;
    const uint4 v = load_chunk(text, base, n, valid);
    const unsigned quotes = unescaped_quotes(text, base, v, valid);
    int total;
    const int before = block_exclusive_scan<kTextWaves>(__popc(quotes), red, total);
    unsigned in_string = (unsigned)(tile_quotes[blockIdx.x] + before) & 1u;
    // a token starts at a token byte outside strings whose predecessor is no token byte (inside a string it could not be: the
    // string state changes at quotes only)
    bool prev_num = valid > 0 && base > 0 && json_is_number_byte(text[base - 1]);
    uint4 out = make_uint4(0, 0, 0, 0);
    int n_tok = 0, n_brk = 0, n_nonnum = 0, depth = 0;
#pragma unroll
    for (int k = 0; k < kLaneBytes; ++k) {
        if (k < valid) {
            const unsigned char c = (unsigned char)byte_of(v, k);
            unsigned code;
            if ((quotes >> k) & 1u) {
                in_string ^= 1u;
                code = kNonNum;
            } else if (in_string) {
                code = kNonNum;
            } else if (c == '[') {
                code = kOpen;
            } else if (c == ']') {
                code = kClose;
            } else if (c == ',') {
                code = kComma;
            } else if (is_ws(c)) {
                code = kWs;
            } else if (json_is_number_byte(c)) {
                code = prev_num ? kNum : kNumStart;
            } else {
                code = kNonNum;
            }
            prev_num = json_is_number_byte(c);
            n_tok += code == kNumStart;
            n_brk += code == kOpen || code == kClose;
            n_nonnum += code == kNonNum;
            depth += (code == kOpen) - (code == kClose);
            put_byte(out, k, code);
        }
    }
    store_chunk(cls, base, valid, out);
    n_tok = block_sum<kTextWaves>(n_tok, red);
    n_brk = block_sum<kTextWaves>(n_brk, red);
    n_nonnum = block_sum<kTextWaves>(n_nonnum, red);
    depth = block_sum<kTextWaves>(depth, red);
    if (threadIdx.x == 0) {
        tile_totals[0 * (size_t)ntiles + blockIdx.x] = n_tok;
        tile_totals[1 * (size_t)ntiles + blockIdx.x] = n_brk;
        tile_totals[2 * (size_t)ntiles + blockIdx.x] = n_nonnum;
        tile_totals[3 * (size_t)ntiles + blockIdx.x] = depth;
    }
}

struct JsonLists {
    int *tok_pos, *tok_brk, *brk_pos, *brk_key, *brk_nonnum, *brk_tok;
    long long tok_cap, brk_cap;
};

__global__ __launch_bounds__(kLanes) void json_compact_kernel(const unsigned char* __restrict__ cls, long long n, int ntiles,
                                                              const int* __restrict__ tile_before, JsonLists out) {
    __shared__ int red[kTextWaves];
    const long long base = (long long)blockIdx.x * DAD3D_JSON_PARSE_TILE_BYTES + threadIdx.x * kLaneBytes;
    int valid;
    const uint4 v = load_chunk(cls, base, n, valid);
    int n_tok = 0, n_brk = 0, n_nonnum = 0, d = 0;
#pragma unroll
    for (int k = 0; k < kLaneBytes; ++k) {
        const unsigned code = byte_of(v, k);  // bytes behind n read as 0 = whitespace
        n_tok += code == kNumStart;
        n_brk += code == kOpen || code == kClose;
        n_nonnum += code == kNonNum;
        d += (code == kOpen) - (code == kClose);
    }
    int total;
    long long tok = (long long)tile_before[0 * (size_t)ntiles + blockIdx.x] + block_exclusive_scan<kTextWaves>(n_tok, red, total);
    long long brk = (long long)tile_before[1 * (size_t)ntiles + blockIdx.x] + block_exclusive_scan<kTextWaves>(n_brk, red, total);
    int nonnum = tile_before[2 * (size_t)ntiles + blockIdx.x] + block_exclusive_scan<kTextWaves>(n_nonnum, red, total);
    int depth = tile_before[3 * (size_t)ntiles + blockIdx.x] + block_exclusive_scan<kTextWaves>(d, red, total);
#pragma unroll 1  // 16 copies of the divergent stores below cost more registers than the loop saves
    for (int k = 0; k < kLaneBytes; ++k) {
        const unsigned code = byte_of(v, k);
        if (code == kNumStart) {
            if (tok < out.tok_cap) {
                out.tok_pos[tok] = (int)(base + k);
                out.tok_brk[tok] = (int)brk;
            }
            ++tok;
        } else if (code == kOpen || code == kClose) {
            depth += code == kOpen;  // the depth inside: a `[` and its `]` get the same key
            if (brk < out.brk_cap) {
                out.brk_pos[brk] = (int)(base + k);
                out.brk_key[brk] = depth;
                out.brk_nonnum[brk] = nonnum;
                out.brk_tok[brk] = (int)tok;
            }
            depth -= code == kClose;
            ++brk;
        } else if (code == kNonNum) {
            ++nonnum;
        }
    }
}

// with whitespace skipped: `[` in front of the element that starts at p, or `,` with a token or `]` in front of it
__device__ inline bool element_front_ok(const unsigned char* __restrict__ text, long long p) {
    long long j = p - 1;
    while (j >= 0 && is_ws(text[j])) --j;
    if (j < 0) return false;
    if (text[j] == '[') return true;
    if (text[j] != ',') return false;
    --j;
    while (j >= 0 && is_ws(text[j])) --j;
    return j >= 0 && (json_is_number_byte(text[j]) || text[j] == ']');
}

// with whitespace skipped: `,` or `]` behind the element that ends in front of e
__device__ inline bool element_back_ok(const unsigned char* __restrict__ text, long long e, long long n) {
    while (e < n && is_ws(text[e])) ++e;
    return e < n && (text[e] == ',' || text[e] == ']');
}

// with whitespace skipped: no `,` in front of the `]` at p
__device__ inline bool close_front_ok(const unsigned char* __restrict__ text, long long p) {
    long long j = p - 1;
    while (j >= 0 && is_ws(text[j])) --j;
    return j >= 0 && text[j] != ',';
}

__device__ inline long long token_end(const unsigned char* __restrict__ text, long long p, long long n) {
    while (p < n && json_is_number_byte(text[p])) ++p;
    return p;
}

struct JsonCheckArgs {
    const unsigned char* text;
    const int *tok_pos, *tok_brk, *brk_pos, *brk_key, *brk_tok, *arr_open, *arr_close;
    int* arr_rows;
    long long n, n_tokens, n_brackets;
};

__global__ __launch_bounds__(kLanes) void json_check_arrays_kernel(JsonCheckArgs a) {
    const int tid = threadIdx.x;
    const long long oi = a.arr_open[blockIdx.x], ci = a.arr_close[blockIdx.x];
    if (oi < 0 || ci >= a.n_brackets || oi >= ci) {  // uniform over the workgroup
        if (tid == 0) a.arr_rows[blockIdx.x] = -1;
        return;
    }
    const int key = a.brk_key[oi];
    const long long t0 = a.brk_tok[oi], t1 = a.brk_tok[ci], count = t1 - t0, inner = ci - oi - 1;
    const long long close_pos = a.brk_pos[ci];
    const long long rows = inner / 2;
    int bad = count <= 0 || t0 < 0 || t1 > a.n_tokens || (inner & 1) || close_pos < 0 || close_pos >= a.n;
    if (rows > 0 && count % rows != 0) bad = 1;
    const long long per_row = rows > 0 && !bad ? count / rows : 1;
    if (bad) {  // uniform
        if (tid == 0) a.arr_rows[blockIdx.x] = -1;
        return;
    }
    // inner brackets: all one level down, `[` and `]` in turn, well separated
    for (long long j = oi + 1 + tid; j < ci; j += kLanes) {
        const long long p = a.brk_pos[j];
        if (p < 0 || p >= a.n || a.brk_key[j] != key + 1) {
            bad = 1;
            continue;
        }
        const bool open = a.text[p] == '[';
        if (open != (((j - oi - 1) & 1) == 0)) bad = 1;
        if (open) {
            if (!element_front_ok(a.text, p)) bad = 1;
        } else {
            if (!close_front_ok(a.text, p) || !element_back_ok(a.text, p + 1, a.n)) bad = 1;
        }
    }
    if (tid == 0 && !close_front_ok(a.text, close_pos)) bad = 1;
    for (long long t = t0 + tid; t < t1; t += kLanes) {
        const long long p = a.tok_pos[t];
        if (p < 0 || p >= a.n) {
            bad = 1;
            continue;
        }
        const long long e = token_end(a.text, p, a.n);
        unsigned long long bits;
        int is_int;
        if (json_parse_number(a.text, p, e, bits, is_int)) bad = 1;
        if (!element_front_ok(a.text, p) || !element_back_ok(a.text, e, a.n)) bad = 1;
        if (rows > 0) {  // inside a row (an odd number of inner brackets in front), and the row its ordinal says
            const long long in_front = (long long)a.tok_brk[t] - oi - 1;
            if (!(in_front & 1) || (in_front - 1) / 2 != (t - t0) / per_row) bad = 1;
        }
    }
    bad = __syncthreads_or(bad);
    if (tid == 0) a.arr_rows[blockIdx.x] = bad ? -1 : (int)rows;
}

__global__ __launch_bounds__(kLanes) void json_values_kernel(const unsigned char* __restrict__ text, long long n, const int* __restrict__ tok_pos,
                                                             long long n_tokens, const int* __restrict__ records, long long n_records,
                                                             long long n_values, unsigned long long* __restrict__ values,
                                                             unsigned char* __restrict__ is_int_out) {
    const long long v = (long long)blockIdx.x * kLanes + threadIdx.x;
    if (v >= n_values) return;
    long long lo = 0, hi = n_records - 1;  // the last record whose first value index is <= v
    while (lo < hi) {
        const long long mid = (lo + hi + 1) >> 1;
        if (records[mid * DAD3D_JSON_PARSE_RECORD_INTS + 2] <= v) lo = mid;
        else hi = mid - 1;
    }
    const int* r = records + lo * DAD3D_JSON_PARSE_RECORD_INTS;
    const long long k = v - r[2], t = (long long)r[5] + k;
    unsigned long long bits = 0;
    int is_int = 0;
    if (k >= 0 && k < r[3] && t >= 0 && t < n_tokens) {
        const long long p = tok_pos[t];
        if (p >= 0 && p < n && json_parse_number(text, p, token_end(text, p, n), bits, is_int)) bits = 0, is_int = 0;
    }
    values[v] = bits;
    is_int_out[v] = (unsigned char)is_int;
}

size_t cls_bytes(long long n) { return ((size_t)n + 15) / 16 * 16; }

}  // namespace

int json_parse_tiles(long long n_bytes) { return (int)((n_bytes + DAD3D_JSON_PARSE_TILE_BYTES - 1) / DAD3D_JSON_PARSE_TILE_BYTES); }

size_t json_parse_scratch_bytes(long long n_bytes) { return cls_bytes(n_bytes) + (size_t)json_parse_tiles(n_bytes) * 5 * sizeof(int); }

dad3d_status launch_json_parse_index(const unsigned char* text, long long n, void* scratch, int* counts, hipStream_t s) {
    const int ntiles = json_parse_tiles(n);
    unsigned char* cls = static_cast<unsigned char*>(scratch);
    int* tile_quotes = reinterpret_cast<int*>(cls + cls_bytes(n));
    int* tile_totals = tile_quotes + ntiles;
    hipLaunchKernelGGL(json_tile_quotes_kernel, dim3(ntiles), dim3(kLanes), 0, s, text, n, tile_quotes);
    DAD3D_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(json_scan_tiles_kernel, dim3(1), dim3(kLanes), 0, s, tile_quotes, ntiles, 1, static_cast<int*>(nullptr));
    DAD3D_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(json_classify_kernel, dim3(ntiles), dim3(kLanes), 0, s, text, n, ntiles, tile_quotes, cls, tile_totals);
    DAD3D_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(json_scan_tiles_kernel, dim3(1), dim3(kLanes), 0, s, tile_totals, ntiles, 4, counts);
    DAD3D_HIP_TRY(hipGetLastError());
    return DAD3D_OK;
}

dad3d_status launch_json_parse_lists(const JsonParseListsArgs& a, hipStream_t s) {
    const int ntiles = json_parse_tiles(a.n_bytes);
    const unsigned char* cls = static_cast<const unsigned char*>(a.scratch);
    const int* tile_before = reinterpret_cast<const int*>(cls + cls_bytes(a.n_bytes)) + ntiles;
    JsonLists out{a.tok_pos, a.tok_brk, a.brk_pos, a.brk_key, a.brk_nonnum, a.brk_tok, a.tok_cap, a.brk_cap};
    hipLaunchKernelGGL(json_compact_kernel, dim3(ntiles), dim3(kLanes), 0, s, cls, a.n_bytes, ntiles, tile_before, out);
    DAD3D_HIP_TRY(hipGetLastError());
    return DAD3D_OK;
}

dad3d_status launch_json_parse_check_arrays(const JsonParseCheckArgs& a, hipStream_t s) {
    JsonCheckArgs k{a.text, a.tok_pos, a.tok_brk, a.brk_pos, a.brk_key, a.brk_tok, a.arr_open, a.arr_close, a.arr_rows, a.n_bytes, a.n_tokens, a.n_brackets};
    hipLaunchKernelGGL(json_check_arrays_kernel, dim3((unsigned)a.n_arrays), dim3(kLanes), 0, s, k);
    DAD3D_HIP_TRY(hipGetLastError());
    return DAD3D_OK;
}

dad3d_status launch_json_parse_extract(const JsonParseExtractArgs& a, hipStream_t s) {
    const unsigned blocks = (unsigned)((a.n_values + kLanes - 1) / kLanes);
    hipLaunchKernelGGL(json_values_kernel, dim3(blocks), dim3(kLanes), 0, s, a.text, a.n_bytes, a.tok_pos, a.n_tokens, a.records, a.n_records,
                       a.n_values, reinterpret_cast<unsigned long long*>(a.values), a.is_int);
    DAD3D_HIP_TRY(hipGetLastError());
    return DAD3D_OK;
}

void json_parse_number_host(const unsigned char* text, const long long* starts, const long long* ends, size_t n, unsigned long long* bits,
                            unsigned char* is_int, unsigned* flags) {
    for (size_t i = 0; i < n; ++i) {
        int integer = 0;
        flags[i] = ends[i] < starts[i] ? (unsigned)DAD3D_JSON_PARSE_FLAG_GRAMMAR : json_parse_number(text, starts[i], ends[i], bits[i], integer);
        if (flags[i]) bits[i] = 0;
        is_int[i] = (unsigned char)integer;
    }
}

}  // namespace dad3d
