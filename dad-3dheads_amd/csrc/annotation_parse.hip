// DAD-3DHeads annotation files read on the device: a batch of JSON documents -> vertices [B,N,3], model-view [B,16] and
// projection [B,16] in float32, the arrays FlameDataset._load_mesh makes (model_training/data/flame_dataset.py:115-127), plus one status
// word per document. Status 0 means the device validated every byte of the document; any DAD3D_ANNOTATION_FLAG_* bit hands it to json.load.
//
// One workgroup of 256 lanes per document walks its tiles of 4096 bytes in order; nothing is shared between documents, so a broken one
// cannot shift the string state of its neighbours. A lane holds 16 consecutive bytes in four registers. Per tile:
//   A  unescaped quotes (a quote behind an even run of backslashes; the look back only reads and is capped)  -> scan -> string state
//   B  the class of every byte by selects, kept as bit masks per lane (tokens, opens, closes, numbers, words) -> scan -> ordinal, depth
//      the kinds of the tile's tokens go to LDS by ordinal, behind the two the workgroup carried in
//   C  every token is legal or not given its kind, the two tokens in front of it and its depth; depth-1 keys  -> scans -> counts
//      a key's record {name, token ordinal, numbers and rows in front of it} goes to LDS by ordinal, behind the one carried in
//   D  no backslash in a key; the shape of the three values from counts relative to their key's record
//   E  the words: true / false / null, and number tokens through json_parse_number; a number in its place is stored as float32
// The workgroup carries from tile to tile: quote parity, depth, the last two token kinds, the last key record and the running counts.
// Sums and scans are those of collectives.hpp; every store is a plain vector store with one writer; no atomics, no waiting on others.
#include "common.hpp"
#include "json_parse_number.hpp"
#include "text_tile.hpp"

namespace dad3d {
namespace {

constexpr int kLanes = kTextTile;
constexpr int kLaneBytes = kTextLaneBytes;
constexpr int kTile = kLanes * kLaneBytes;
static_assert(kTile == DAD3D_JSON_PARSE_TILE_BYTES, "a tile is one 16-byte chunk per lane");
constexpr int kKeyCap = kTile / 3 + 2;  // a key takes three bytes at least (`"",`); slot 0 is the record carried in

enum : unsigned { tNone = 0, tLBrace, tRBrace, tLBrack, tRBrack, tComma, tColon, tString, tNumber, tLiteral };
enum : unsigned {
    fGrammar = DAD3D_ANNOTATION_FLAG_GRAMMAR,
    fKeys = DAD3D_ANNOTATION_FLAG_KEYS,
    fShape = DAD3D_ANNOTATION_FLAG_SHAPE,
    fNumber = DAD3D_ANNOTATION_FLAG_NUMBER,
    fString = DAD3D_ANNOTATION_FLAG_STRING,
    fRange = DAD3D_ANNOTATION_FLAG_RANGE
};

struct OpOr {
    template <typename T>
    __device__ static __forceinline__ T of(T a, T b) { return a | b; }
};

__device__ inline bool is_word(unsigned char c) {
    return (c >= '0' && c <= '9') || (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') || c == '+' || c == '-' || c == '.';
}

// backslashes right in front of byte i, counted up to DAD3D_ANNOTATION_MAX_BACKSLASH_RUN; reads only, ends at byte 0 of the document
__device__ inline int backslashes_before(const unsigned char* __restrict__ d, long long i) {
    int r = 0;
    while (r < DAD3D_ANNOTATION_MAX_BACKSLASH_RUN && i - 1 - r >= 0 && d[i - 1 - r] == '\\') ++r;
    return r;
}

__device__ inline bool text_is(const unsigned char* __restrict__ d, long long at, long long n, const char* word, int len) {
    if (at + len > n) return false;
    for (int j = 0; j < len; ++j)
        if (d[at + j] != (unsigned char)word[j]) return false;
    return true;
}

// the string that opens at byte i: 1 "vertices", 2 "model_view_matrix", 3 "projection_matrix", 0 anything else
__device__ inline int key_name(const unsigned char* __restrict__ d, long long i, long long n) {
    const unsigned char c = i + 1 < n ? d[i + 1] : 0;
    const char* name = c == 'v' ? "vertices\"" : c == 'm' ? "model_view_matrix\"" : "projection_matrix\"";
    return text_is(d, i + 1, n, name, c == 'v' ? 9 : 18) ? (c == 'v' ? 1 : c == 'm' ? 2 : 3) : 0;
}

// FNV-1a of the key that opens at byte i, up to its closing quote; a key whose quote is not among the DAD3D_ANNOTATION_MAX_KEY_BYTES + 1
// bytes behind the opening one is flagged. Two keys with one hash count as one key twice: unsure goes to the host
__device__ inline unsigned key_hash(const unsigned char* __restrict__ d, long long i, long long n, unsigned& flags) {
    unsigned h = 2166136261u;
    for (int j = 0; j <= DAD3D_ANNOTATION_MAX_KEY_BYTES && i + 1 + j < n; ++j) {
        const unsigned char c = d[i + 1 + j];
        if (c == '"') return h;
        h = (h ^ c) * 16777619u;
    }
    flags |= fKeys;
    return h;
}

// the word d[0, len) is true, false or null
__device__ inline bool is_literal(const unsigned char* __restrict__ d, int len) {
    if (len != 4 && len != 5) return false;
    unsigned long long w = 0;
    for (int j = 0; j < len; ++j) w |= (unsigned long long)d[j] << (8 * j);
    return w == 0x65757274ull || w == 0x6c6c756eull || w == 0x65736c6166ull;  // little-endian "true", "null", "false"
}

__device__ inline unsigned code_of(unsigned lo, unsigned hi, int k) { return ((k < 8 ? lo : hi) >> (4 * (k & 7))) & 15u; }

// a value ended in front of a `,` or a closing bracket at depth d: p1, p2 = the two tokens in front of it
__device__ inline bool value_ended(unsigned p1, unsigned p2, int d) {
    if (p1 == tNumber || p1 == tLiteral || p1 == tRBrack) return true;
    return p1 == tString && (d >= 2 || p2 == tColon);  // at depth 1 a string is a value only behind a colon
}

__device__ inline bool token_legal(unsigned k, unsigned p1, unsigned p2, int d) {
    if (p1 == tNone) return k == tLBrace;
    if (p1 == tRBrace || k == tLBrace) return false;  // nothing behind the closing brace; no object below the document itself
    switch (k) {
        case tString: return d == 1 ? (p1 == tLBrace || p1 == tComma || p1 == tColon) : d >= 2 && (p1 == tLBrack || p1 == tComma);
        case tNumber:
        case tLiteral:
        case tLBrack: return d == 1 ? p1 == tColon : d >= 2 && (p1 == tLBrack || p1 == tComma);
        case tColon: return d == 1 && p1 == tString && (p2 == tLBrace || p2 == tComma);
        case tComma: return d >= 1 && value_ended(p1, p2, d);
        case tRBrack: return d >= 2 && (p1 == tLBrack || value_ended(p1, p2, d));
        case tRBrace: return d == 1 && value_ended(p1, p2, 1);
        default: return false;
    }
}

// the three outputs of a flagged document; behind a barrier, so the values some lanes stored before are gone
__device__ inline void fill_nan(float* const* out_of, const long long* count_of, int tid) {
    const float nan = __int_as_float(0x7fc00000);
    for (int r = 1; r <= 3; ++r)
        for (long long i = tid; i < count_of[r]; i += kLanes) out_of[r][i] = nan;
}

struct AnnotationArgs {
    const unsigned char* text;
    long long n_bytes;
    const long long *offsets, *sizes;
    int n_verts;
    float *vertices, *model_view, *projection;
    int* status;
};

__global__ __launch_bounds__(kLanes) void annotation_parse_kernel(AnnotationArgs a) {
    __shared__ int red[kTextWaves];
    __shared__ unsigned char toks[2 + kTile];  // [0], [1]: the two tokens carried in; [2 + i]: token i of the tile
    __shared__ int4 keys[kKeyCap];             // {name, token ordinal, numbers in front, rows in front}; [0] carried in
    __shared__ unsigned char live[kKeyCap];    // the name where it is its first appearance, else 0
    __shared__ unsigned key_hashes[kKeyCap];   // the hash of the tile's key i at [1 + i]
    __shared__ unsigned seen_hashes[DAD3D_ANNOTATION_MAX_KEYS];  // of the document's keys so far, in order
    __shared__ float* out_of[4];               // [1] vertices, [2] model-view, [3] projection of this document: read where a value is
    __shared__ long long count_of[4];          // stored, so that they take no scalar registers across the walk
    __shared__ int* status_of;                 // its status word, for the same reason
    const int tid = threadIdx.x, doc = blockIdx.x;
    const long long off = a.offsets[doc], size = a.sizes[doc];
    if (tid == 0) {
        out_of[1] = a.vertices + (size_t)doc * a.n_verts * 3, count_of[1] = (long long)a.n_verts * 3;
        out_of[2] = a.model_view + (size_t)doc * 16, count_of[2] = 16;
        out_of[3] = a.projection + (size_t)doc * 16, count_of[3] = 16;
        status_of = a.status + doc;
    }
    __syncthreads();
    unsigned flags = 0, done = 0;
    if (!(off >= 0 && (off & 15) == 0 && size >= 0 && size <= 0x7fffffffLL && off <= a.n_bytes && size <= a.n_bytes - off)) {  // uniform
        fill_nan(out_of, count_of, tid);
        if (tid == 0) *status_of = (int)fRange;
        return;
    }
    // uniform over the workgroup
    int parity = 0, depth = 0, tok_base = 0, num_base = 0, row_base = 0, key_base = 0;
    unsigned t1 = tNone, t2 = tNone, seen = 0;
    int4 key_in = make_int4(0, -2, 0, 0);
    unsigned live_in = 0;
    const unsigned char* __restrict__ d = a.text + off;
    const long long n = size;
    const int ntiles = __builtin_amdgcn_readfirstlane((int)((size + kTile - 1) / kTile));  // the same in every lane: a scalar loop

    for (int tile = 0; tile < ntiles; ++tile) {
        const long long base = (long long)tile * kTile + tid * kLaneBytes;
        int valid;
        const uint4 v = load_chunk(d, base, n, valid);

        // A: quotes and escaping backslashes. The candidates come from compares; only they look back (rare in these files)
        unsigned candidates = 0, is_quote = 0;
#pragma unroll
        for (int k = 0; k < kLaneBytes; ++k) {
            const unsigned c = byte_of(v, k);
            candidates |= (unsigned)(k < valid && (c == '"' || c == '\\')) << k;
            is_quote |= (unsigned)(c == '"') << k;
        }
        unsigned quotes = 0, escaping = 0;
        for (unsigned m = candidates; m; m &= m - 1) {
            const int k = __ffs(m) - 1;
            const int run = backslashes_before(d, base + k);
            if (run == DAD3D_ANNOTATION_MAX_BACKSLASH_RUN) flags |= fString;
            if ((run & 1) == 0) ((is_quote >> k) & 1u ? quotes : escaping) |= 1u << k;
        }
        int total_quotes;
        const unsigned string_in = (unsigned)(parity + block_exclusive_scan<kTextWaves>((int)__popc(quotes), red, total_quotes)) & 1u;
        if (tid == 0) {
            toks[0] = (unsigned char)t2, toks[1] = (unsigned char)t1;
            keys[0] = key_in, live[0] = (unsigned char)live_in;
        }
        // bit k: byte k lies behind an odd number of quotes (counted from the document's start, itself excluded)
        unsigned odd = quotes << 1;
        odd ^= odd << 1, odd ^= odd << 2, odd ^= odd << 4, odd ^= odd << 8;
        if (string_in) odd = ~odd;

        // B: classes, with selects only
        bool prev_word = valid > 0 && base > 0 && is_word(d[base - 1]);
        unsigned lo = 0, hi = 0, backslash = 0, open_mask = 0, close_mask = 0, num_mask = 0, word_mask = 0, token_mask = 0;
#pragma unroll 1  // unrolled, the sixteen bytes' compare masks outnumber the scalar registers
        for (int k = 0; k < kLaneBytes; ++k) {
            const unsigned char c = (unsigned char)byte_of(v, k);
            const bool here = k < valid, quote = (quotes >> k) & 1u, inside = (odd >> k) & 1u;
            const bool content = here && inside && !quote, plain = here && !inside && !quote;
            const bool word = plain && is_word(c);
            unsigned code = tNone;
            code = c == '{' ? (unsigned)tLBrace : code;
            code = c == '}' ? (unsigned)tRBrace : code;
            code = c == '[' ? (unsigned)tLBrack : code;
            code = c == ']' ? (unsigned)tRBrack : code;
            code = c == ',' ? (unsigned)tComma : code;
            code = c == ':' ? (unsigned)tColon : code;
            code = word && !prev_word ? (((c >= '0' && c <= '9') || c == '-') ? (unsigned)tNumber : (unsigned)tLiteral) : code;
            if (plain && code == tNone && !word && !is_ws(c)) flags |= fGrammar;
            code = plain ? code : tNone;
            code = here && quote && !inside ? (unsigned)tString : code;
            if (content && (c < 0x20 || c > 0x7e)) flags |= fString;
            backslash |= (unsigned)(content && c == '\\') << k;
            prev_word = word;
            token_mask |= (unsigned)(code != tNone) << k;
            open_mask |= (unsigned)(code == tLBrace || code == tLBrack) << k;
            close_mask |= (unsigned)(code == tRBrace || code == tRBrack) << k;
            num_mask |= (unsigned)(code == tNumber) << k;
            word_mask |= (unsigned)(code == tNumber || code == tLiteral) << k;
            if (k < 8) lo |= code << (4 * (k & 7));
            else hi |= code << (4 * (k & 7));
        }
        for (unsigned m = escaping & backslash; m; m &= m - 1) {  // what an escaping backslash escapes
            const long long at = base + __ffs(m);
            const unsigned char e = at < n ? d[at] : 0;
            if (!(e == '"' || e == '\\' || e == '/' || e == 'b' || e == 'f' || e == 'n' || e == 'r' || e == 't')) flags |= fString;
        }
        const int n_tok = __popc(token_mask), delta = __popc(open_mask) - __popc(close_mask);
        int total2;
        const int before2 = block_exclusive_scan<kTextWaves>(n_tok + delta * 65536, red, total2);
        const int tok_before = before2 & 0xffff, depth_before = depth + (before2 - tok_before) / 65536;
        const int total_tok = total2 & 0xffff, total_delta = (total2 - total_tok) / 65536;
        {
            int j = 0;
            for (unsigned m = token_mask; m; m &= m - 1) toks[2 + tok_before + j++] = (unsigned char)code_of(lo, hi, __ffs(m) - 1);
        }
        __syncthreads();

        // C: legality, keys, counts. What stands in front of byte k in this lane comes from the masks below bit k
        unsigned key_mask = 0, row_mask = 0;
        for (unsigned m = token_mask; m; m &= m - 1) {
            const int k = __ffs(m) - 1;
            const unsigned below = (1u << k) - 1u, code = code_of(lo, hi, k);
            const int at = 2 + tok_before + __popc(token_mask & below);
            const int dep = depth_before + __popc(open_mask & below) - __popc(close_mask & below);
            const unsigned p1 = toks[at - 1], p2 = toks[at - 2];
            if (!token_legal(code, p1, p2, dep)) flags |= fGrammar;
            key_mask |= (unsigned)(code == tString && dep == 1 && (p1 == tLBrace || p1 == tComma)) << k;
            row_mask |= (unsigned)(code == tLBrack && dep == 2) << k;
        }
        const int n_key = __popc(key_mask);
        int total3, total_key;
        const int before3 = block_exclusive_scan<kTextWaves>(__popc(num_mask) + __popc(row_mask) * 65536, red, total3);
        const int key_before = block_exclusive_scan<kTextWaves>(n_key, red, total_key);
        const int num_before = before3 & 0xffff, row_before = before3 >> 16;
        for (unsigned m = key_mask; m; m &= m - 1) {
            const int k = __ffs(m) - 1;
            const unsigned below = (1u << k) - 1u;
            const int slot = 1 + key_before + __popc(key_mask & below);
            key_hashes[slot] = key_hash(d, base + k, n, flags);
            keys[slot] =
                make_int4(key_name(d, base + k, n), tok_base + tok_before + __popc(token_mask & below),
                          num_base + num_before + __popc(num_mask & below), row_base + row_before + __popc(row_mask & below));
        }
        __syncthreads();
        for (int e = 0; e < n_key; ++e) {  // a name counts where it appears first
            const int slot = 1 + key_before + e, name = keys[slot].x;
            bool again = name != 0 && ((seen >> name) & 1u);
            for (int s = 1; s < slot && name != 0; ++s) again = again || keys[s].x == name;
            // no key twice: not among the tile's keys in front of it, nor among the document's before the tile
            const unsigned hash = key_hashes[slot];
            const int known = min(key_base, DAD3D_ANNOTATION_MAX_KEYS), order = key_base + slot - 1;
            for (int s = 1; s < slot; ++s) again = again || key_hashes[s] == hash;
            for (int s = 0; s < known; ++s) again = again || seen_hashes[s] == hash;
            if (order < DAD3D_ANNOTATION_MAX_KEYS) seen_hashes[order] = hash;  // behind everything a lane of this tile reads
            if (again || order >= DAD3D_ANNOTATION_MAX_KEYS) flags |= fKeys;
            live[slot] = (unsigned char)(again ? 0 : name);
        }
        __syncthreads();

        // D: no backslash in a key, and the shapes of the three values
        for (unsigned m = backslash; m; m &= m - 1) {
            const unsigned below = (1u << (__ffs(m) - 1)) - 1u;
            // the last key in front of this byte opened the last token in front of it: the backslash stands inside the key
            if (keys[key_before + __popc(key_mask & below)].y + 1 == tok_base + tok_before + __popc(token_mask & below)) flags |= fKeys;
        }
        for (unsigned m = token_mask & ~key_mask; m; m &= m - 1) {
            const int k = __ffs(m) - 1;
            const unsigned below = (1u << k) - 1u, code = code_of(lo, hi, k);
            const int slot = key_before + __popc(key_mask & below), region = live[slot];
            if (!region) continue;
            const int4 key = keys[slot];
            const int dep = depth_before + __popc(open_mask & below) - __popc(close_mask & below);
            const long long nr = (long long)num_base + num_before + __popc(num_mask & below) - key.z;
            const long long rr = (long long)row_base + row_before + __popc(row_mask & below) - key.w;
            const long long width = region == 1 ? 3 : 4, height = region == 1 ? count_of[1] / 3 : 4;
            const bool word = code == tNumber || code == tLiteral, text = code == tString || code == tLiteral;
            bool bad = (dep == 1 && (word || text)) || (dep >= 2 && text) || (code == tNumber && dep != 3);
            bad = bad || (code == tLBrack && (dep >= 3 || (dep == 2 && nr != width * rr)));
            bad = bad || (code == tRBrack && (dep >= 4 || (dep == 3 && nr != width * rr)));
            const bool closes = code == tRBrack && dep == 2, whole = rr == height && nr == width * height;
            if (bad || (closes && !whole)) flags |= fShape;
            if (closes && whole) done |= 1u << region;
        }
        // E: the words. A number token goes through the number routine wherever it stands; one in its place is stored.
        // Positions are 32-bit here (a document is shorter than 2^31 bytes): 64-bit compares take scalar registers for their carries
        for (unsigned m = word_mask; m; m &= m - 1) {
            const int k = __ffs(m) - 1;
            const unsigned below = (1u << k) - 1u;
            const bool number = (num_mask >> k) & 1u;
            const int dep = depth_before + __popc(open_mask & below) - __popc(close_mask & below);
            const unsigned i = (unsigned)base + k, size = (unsigned)n;
            unsigned end = i;
            while (end < size && end - i <= DAD3D_ANNOTATION_MAX_WORD_BYTES && is_word(d[end])) ++end;
            unsigned long long bits = 0;
            int is_int = 0;
            unsigned why;
            if (end - i > DAD3D_ANNOTATION_MAX_WORD_BYTES) why = fGrammar;
            else if (!number) why = is_literal(d + i, (int)(end - i)) ? 0u : (unsigned)fGrammar;
            else why = json_parse_number(d + i, 0, end - i, bits, is_int) ? (unsigned)fNumber : 0u;
            flags |= why;
            const int slot = key_before + __popc(key_mask & below), region = live[slot];
            const int nr = num_base + num_before + __popc(num_mask & below) - keys[slot].z;
            if (number && !why && region && dep == 3 && nr >= 0 && nr < (int)count_of[region]) {
                if (is_int && (bits << 1) == 0) bits = 0;  // `-0` is the int 0
                out_of[region][nr] = (float)__longlong_as_double((long long)bits);
            }
        }

        // the words carried to the next tile (every lane the same)
        parity = (parity + total_quotes) & 1;
        depth += total_delta;
        t2 = toks[2 + total_tok - 2], t1 = toks[2 + total_tok - 1];
        for (int s = 1; s <= total_key; ++s) seen |= 1u << keys[s].x;
        key_in = keys[total_key], live_in = live[total_key];
        tok_base += total_tok, num_base += total3 & 0xffff, row_base += total3 >> 16, key_base += total_key;
        // the scans of the next tile put their barriers between these reads and its writes
    }

    if (parity || depth != 0 || t1 != tRBrace) flags |= fGrammar;
    if ((seen & 0xeu) != 0xeu) flags |= fKeys;
    __shared__ unsigned red_or[kTextWaves];
    const unsigned all = block_reduce<OpOr, kTextWaves>(flags | done << 8, red_or);
    unsigned status = all & 0xffu;
    if ((all >> 8 & 0xeu) != 0xeu) status |= fShape;
    if (status) fill_nan(out_of, count_of, tid);  // never left unwritten, never half a document
    if (tid == 0) *status_of = (int)status;
}

}  // namespace

dad3d_status launch_annotation_parse(const AnnotationParseArgs& p, hipStream_t s) {
    AnnotationArgs a{p.text, p.n_bytes, p.doc_offsets, p.doc_sizes, p.n_verts, p.vertices, p.model_view, p.projection, p.status};
    hipLaunchKernelGGL(annotation_parse_kernel, dim3((unsigned)p.batch), dim3(kLanes), 0, s, a);
    DAD3D_HIP_TRY(hipGetLastError());
    return DAD3D_OK;
}

}  // namespace dad3d
