// The vertex block of a Wavefront .obj as MeshSaver writes it (demo_utils.py:130-144): N lines `v %.8f %.8f %.8f\n` per mesh,
// formatted on the device, byte for byte what Python's '%' operator prints for float(np.float32(x)).
//
// The rule, integers only: a float32 is (-1)^s m 2^e with m < 2^24; P = m 10^8 < 2^51.
//   e >= 0: Q = P << e (exact in 64 bits while e <= 13, |x| < 2^37)      e < 0: Q = P >> -e, rounded half to even
//   text = '-' when the sign bit is set (also -0.0 and negatives that round to zero), Q / 10^8, '.', Q % 10^8 in 8 digits
// Anything else (NaN, inf, |x| >= 2^37) sets the mesh's flag; the host formats that mesh.
//
// Two launches of (tiles, batch) workgroups, a tile = 256 lines = one line per lane:
//   obj_line_lengths_kernel  the byte length of every tile (from the same Q as the text) and its flag bits -> scratch
//   obj_write_text_kernel    sums the tile lengths of its mesh (offset of this tile, length and flag of the mesh), scans its
//                            256 line lengths, writes each line's characters into an LDS image of the tile that starts at
//                            (offset mod 16), and copies the image out in aligned 16-byte stores. Only the up to 15 bytes a
//                            tile shares a 16-byte unit with its neighbour on either end leave as byte stores.
#include "common.hpp"
#include "text_tile.hpp"

namespace dad3d {
namespace {

constexpr int kObjTile = kTextTile;                           // lines per workgroup, one per lane
constexpr int kObjMaxLine = DAD3D_OBJ_MAX_LINE_BYTES;         // "v" + 3 x (" " + "-" + 12 digits + "." + 8 digits) + "\n"
constexpr int kObjStageVecs = (kObjTile * kObjMaxLine + 15 + 15) / 16;  // the tile image: up to 15 bytes of lead-in + the lines

struct ObjNumber {
    unsigned hi, lo;  // integer part = hi * 10^6 + lo, lo < 10^6
    unsigned frac;    // the eight decimals
    int int_digits;
    int neg;
    __device__ int length() const { return neg + int_digits + 9; }
};

__device__ inline int digits_below_1e6(unsigned v) {
    return 1 + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u);
}

// false: outside the domain (*why = DAD3D_OBJ_FLAG_*)
__device__ inline bool obj_number(float x, ObjNumber& n, int& why) {
    const unsigned u = __float_as_uint(x);
    const unsigned be = (u >> 23) & 0xffu, fr = u & 0x7fffffu;
    if (be == 255u) {
        why |= DAD3D_OBJ_FLAG_NONFINITE;
        return false;
    }
    const int e = be ? (int)be - 150 : -149;
    if (e > 13) {
        why |= DAD3D_OBJ_FLAG_LARGE;
        return false;
    }
    const unsigned long long p = (unsigned long long)(be ? fr | 0x800000u : fr) * 100000000ull;
    unsigned long long q;
    if (e >= 0) {
        q = p << e;
    } else if (e <= -64) {
        q = 0;
    } else {
        const int sh = -e;
        q = p >> sh;
        const unsigned long long rem = p & ((1ull << sh) - 1ull), half = 1ull << (sh - 1);
        q += (rem > half) || (rem == half && (q & 1ull));
    }
    const unsigned long long ip = q / 100000000ull;
    n.frac = (unsigned)(q - ip * 100000000ull);
    n.hi = (unsigned)(ip / 1000000ull);
    n.lo = (unsigned)(ip - (unsigned long long)n.hi * 1000000ull);
    n.int_digits = n.hi ? 6 + digits_below_1e6(n.hi) : digits_below_1e6(n.lo);
    n.neg = (int)(u >> 31);
    return true;
}

// the characters of one number into the LDS image at byte p; returns the byte after it
__device__ inline int obj_put_number(unsigned char* s, int p, const ObjNumber& n) {
    if (n.neg) s[p++] = '-';
    int k = p + n.int_digits - 1;
    unsigned v = n.lo;
    if (n.hi) {
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            s[k--] = (unsigned char)('0' + v % 10u);
            v /= 10u;
        }
        v = n.hi;
    }
    do {
        s[k--] = (unsigned char)('0' + v % 10u);
        v /= 10u;
    } while (v);
    p += n.int_digits;
    s[p] = '.';
    unsigned f = n.frac;
#pragma unroll
    for (int i = 8; i >= 1; --i) {
        s[p + i] = (unsigned char)('0' + f % 10u);
        f /= 10u;
    }
    return p + 9;
}

// bitwise OR over the workgroup (__syncthreads_or answers 0 / 1 per call: one call per flag bit)
__device__ inline int block_or_flags(int why) {
    const int nonfinite = __syncthreads_or(why & DAD3D_OBJ_FLAG_NONFINITE), large = __syncthreads_or(why & DAD3D_OBJ_FLAG_LARGE);
    return (nonfinite ? DAD3D_OBJ_FLAG_NONFINITE : 0) | (large ? DAD3D_OBJ_FLAG_LARGE : 0);
}

// the tile's coordinates through LDS: coalesced dword loads, then three conflict-free reads per lane
__device__ inline void load_tile(const float* __restrict__ vertices, size_t first_float, int n_floats, float* sv) {
    for (int i = threadIdx.x; i < n_floats; i += kObjTile) sv[i] = vertices[first_float + i];
    __syncthreads();
}

__global__ __launch_bounds__(kObjTile) void obj_line_lengths_kernel(const float* __restrict__ vertices, int nver, int ntiles,
                                                                     int2* __restrict__ tile_info) {
    __shared__ float sv[kObjTile * 3];
    __shared__ int red[kTextWaves];
    const int tile = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int lines = min(kObjTile, nver - tile * kObjTile);
    load_tile(vertices, ((size_t)b * nver + (size_t)tile * kObjTile) * 3, lines * 3, sv);
    int len = 0, why = 0;
    if (tid < lines) {
        len = 5;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            ObjNumber n;
            if (obj_number(sv[tid * 3 + c], n, why)) len += n.length();
        }
    }
    len = block_sum<kTextWaves>(len, red);
    why = block_or_flags(why);
    if (tid == 0) tile_info[(size_t)b * ntiles + tile] = make_int2(len, why);
}

__global__ __launch_bounds__(kObjTile) void obj_write_text_kernel(const float* __restrict__ vertices, int nver, int ntiles,
                                                                   const int2* __restrict__ tile_info, unsigned char* __restrict__ text,
                                                                   size_t text_stride, long long* __restrict__ lengths,
                                                                   int* __restrict__ flags) {
    __shared__ uint4 stage[kObjStageVecs];
    __shared__ float sv[kObjTile * 3];
    __shared__ int red[kTextWaves];
    const int tile = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;

    // this tile's offset in the mesh's text, the mesh's length and flag: every workgroup sums its mesh's tiles
    int before = 0, total = 0, why = 0;
    for (int t = tid; t < ntiles; t += kObjTile) {
        const int2 info = tile_info[(size_t)b * ntiles + t];
        total += info.x;
        before += t < tile ? info.x : 0;
        why |= info.y;
    }
    before = block_sum<kTextWaves>(before, red);
    total = block_sum<kTextWaves>(total, red);
    why = block_or_flags(why);
    if (tile == 0 && tid == 0) {
        lengths[b] = why ? 0 : total;
        flags[b] = why;
    }
    if (why) return;  // the host formats this mesh

    const int lines = min(kObjTile, nver - tile * kObjTile);
    load_tile(vertices, ((size_t)b * nver + (size_t)tile * kObjTile) * 3, lines * 3, sv);
    ObjNumber n[3];
    int len = 0;
    if (tid < lines) {
        len = 5;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            int unused = 0;
            obj_number(sv[tid * 3 + c], n[c], unused);
            len += n[c].length();
        }
    }
    // exclusive scan of the 256 line lengths. Not block_exclusive_scan of collectives.hpp: its closing barrier costs this kernel
    // 0.6 to 0.9 % (profiles/collectives_refactor_ab.md); here the barrier in front of the copy-out is the only one the scan needs,
    // because `red` is not written again.
    int incl = len;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(incl, d, 64);
        if ((tid & 63) >= d) incl += up;
    }
    if ((tid & 63) == 63) red[tid >> 6] = incl;
    __syncthreads();
    int wave_base = 0;
    for (int w = 0; w < (tid >> 6); ++w) wave_base += red[w];
    static_assert(kTextWaves == 4, "the tile length below adds four wave totals");
    const int tile_len = red[0] + red[1] + red[2] + red[3];

    const int lead = before & 15;  // image byte i is text byte (before - lead) + i: 16-byte units line up
    unsigned char* s = reinterpret_cast<unsigned char*>(stage);
    if (tid < lines) {
        int p = lead + wave_base + incl - len;
        s[p++] = 'v';
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            s[p++] = ' ';
            p = obj_put_number(s, p, n[c]);
        }
        s[p] = '\n';
    }
    __syncthreads();

    // whole 16-byte units as one store each; a unit shared with the neighbouring tile: only this tile's bytes
    copy_tile_out(stage, text + (size_t)b * text_stride + (size_t)(before - lead), lead, lead + tile_len);
}

}  // namespace

size_t obj_format_scratch_bytes(int batch, int nver) { return (size_t)batch * obj_format_tiles(nver) * sizeof(int2); }

dad3d_status launch_obj_format(const ObjFormatArgs& a, hipStream_t s) {
    const int ntiles = obj_format_tiles(a.nver);
    const dim3 grid(ntiles, a.batch);
    int2* info = static_cast<int2*>(a.scratch);
    hipLaunchKernelGGL(obj_line_lengths_kernel, grid, dim3(kObjTile), 0, s, a.vertices, a.nver, ntiles, info);
    DAD3D_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(obj_write_text_kernel, grid, dim3(kObjTile), 0, s, a.vertices, a.nver, ntiles, info, a.text, a.text_stride,
                       reinterpret_cast<long long*>(a.lengths), a.flags);
    DAD3D_HIP_TRY(hipGetLastError());
    return DAD3D_OK;
}

}  // namespace dad3d
