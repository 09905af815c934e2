// JSON text as json.dump writes it, formatted on the device from a layout template: the benchmark submission
// entry (dad_3dheads_benchmark/README.md:78-95) and the demo's flame_params file (demo_utils.py:114-118,147-153).
//
// An item is n_slots float32 values. The template holds the literal bytes in front of every slot (`{"68_landmarks_2d": [[`,
// `, `, `], [`, `]], "N_landmarks_3d": [[`, ...) and the suffix that closes the item (`]]}`); the number in a slot is
// float.__repr__ of the value widened to double (json_number.hpp: integers only). NaN and +-inf set the item's flag; the host
// formats that item.
//
// Two launches of (tiles, batch) workgroups, a tile = 256 slots = one slot per lane, the shape of obj_text.hip:
//   json_slot_lengths_kernel  the byte length of every tile (literals + numbers, + the suffix in the last tile) and its flag -> scratch
//   json_write_text_kernel    sums the tile lengths of its item (offset of this tile, length and flag of the item), scans its 256
//                             slot lengths, writes each slot's literal and number into an LDS image of the tile that starts at
//                             (offset mod 16), and copies the image out in aligned 16-byte stores; only the up to 15 bytes a tile
//                             shares a 16-byte unit with its neighbour on either end leave as byte stores. The last tile appends
//                             the suffix and writes lengths[b] and flags[b].
#include "common.hpp"
#include "json_number.hpp"
#include "text_tile.hpp"

namespace dad3d {
namespace {

constexpr int kJsonTile = kTextTile;  // slots per workgroup, one per lane
constexpr int kJsonMaxSlot = DAD3D_JSON_MAX_LITERAL_BYTES + DAD3D_JSON_MAX_NUMBER_BYTES;
// the tile image: up to 15 bytes of lead-in + the slots + the suffix, in whole 16-byte units
constexpr int kJsonStageVecs = (kJsonTile * kJsonMaxSlot + DAD3D_JSON_MAX_LITERAL_BYTES + 15 + 15) / 16;

// a literal longer than the cap never reaches the kernels through the C ABI; the clamp keeps the LDS image in bounds regardless
__device__ inline int literal_length(const int* __restrict__ offsets, int i) {
    return min(max(offsets[i + 1] - offsets[i], 0), DAD3D_JSON_MAX_LITERAL_BYTES);
}

__global__ __launch_bounds__(kJsonTile) void json_slot_lengths_kernel(const float* __restrict__ values, int n_slots, int ntiles,
                                                                      const int* __restrict__ offsets, int2* __restrict__ tile_info) {
    __shared__ int red[kTextWaves];
    const int tile = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int slot = tile * kJsonTile + tid;
    int len = 0, bad = 0;
    if (slot < n_slots) {
        JsonNumber n;
        len = literal_length(offsets, slot);
        if (json_number(__float_as_uint(values[(size_t)b * n_slots + slot]), n)) {
            len += json_number_length(n);
        } else {
            bad = 1;
        }
    }
    if (tile == ntiles - 1 && tid == kJsonTile - 1) len += literal_length(offsets, n_slots);  // the suffix
    len = block_sum<kTextWaves>(len, red);
    bad = __syncthreads_or(bad);
    if (tid == 0) tile_info[(size_t)b * ntiles + tile] = make_int2(len, bad ? DAD3D_JSON_FLAG_NONFINITE : 0);
}

__global__ __launch_bounds__(kJsonTile) void json_write_text_kernel(const float* __restrict__ values, int n_slots, int ntiles,
                                                                    const int* __restrict__ offsets, const unsigned char* __restrict__ literals,
                                                                    const int2* __restrict__ tile_info, unsigned char* __restrict__ text,
                                                                    size_t text_stride, long long* __restrict__ lengths,
                                                                    int* __restrict__ flags) {
    __shared__ uint4 stage[kJsonStageVecs];
    __shared__ int red[kTextWaves];
    const int tile = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const bool last = tile == ntiles - 1;

    // this tile's offset in the item's text, the item's length and flag: every workgroup sums its item's tiles
    int before = 0, total = 0, why = 0;
    for (int t = tid; t < ntiles; t += kJsonTile) {
        const int2 info = tile_info[(size_t)b * ntiles + t];
        total += info.x;
        before += t < tile ? info.x : 0;
        why |= info.y;
    }
    before = block_sum<kTextWaves>(before, red);
    total = block_sum<kTextWaves>(total, red);
    why = __syncthreads_or(why) ? DAD3D_JSON_FLAG_NONFINITE : 0;
    if (last && tid == 0) {
        lengths[b] = why ? 0 : total;
        flags[b] = why;
    }
    if (why) return;  // the host formats this item

    const int slot = tile * kJsonTile + tid;
    JsonNumber n;
    int lit = 0, lit_at = 0, len = 0;
    if (slot < n_slots) {
        lit_at = offsets[slot];
        lit = literal_length(offsets, slot);
        json_number(__float_as_uint(values[(size_t)b * n_slots + slot]), n);
        len = lit + json_number_length(n);
    }
    int tile_len;
    const int slot_at = block_exclusive_scan<kTextWaves>(len, red, tile_len);

    const int lead = before & 15;  // image byte i is text byte (before - lead) + i: 16-byte units line up
    unsigned char* s = reinterpret_cast<unsigned char*>(stage);
    if (slot < n_slots) {
        unsigned char* p = s + lead + slot_at;
        for (int i = 0; i < lit; ++i) *p++ = literals[lit_at + i];
        json_put_number(p, n);
    }
    if (last) {
        const int suffix = literal_length(offsets, n_slots), suffix_at = offsets[n_slots];
        if (tid < suffix) s[lead + tile_len + tid] = literals[suffix_at + tid];
        tile_len += suffix;
    }
    __syncthreads();

    copy_tile_out(stage, text + (size_t)b * text_stride + (size_t)(before - lead), lead, lead + tile_len);
}

}  // namespace

size_t json_format_scratch_bytes(int batch, int n_slots) { return (size_t)batch * json_format_tiles(n_slots) * sizeof(int2); }

dad3d_status launch_json_format(const JsonFormatArgs& a, hipStream_t s) {
    const int ntiles = json_format_tiles(a.n_slots);
    const dim3 grid(ntiles, a.batch);
    int2* info = static_cast<int2*>(a.scratch);
    // the template image: n_slots + 2 offsets, then the literal bytes
    const int* offsets = static_cast<const int*>(a.literals);
    const unsigned char* bytes = reinterpret_cast<const unsigned char*>(offsets + a.n_slots + 2);
    hipLaunchKernelGGL(json_slot_lengths_kernel, grid, dim3(kJsonTile), 0, s, a.values, a.n_slots, ntiles, offsets, info);
    DAD3D_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(json_write_text_kernel, grid, dim3(kJsonTile), 0, s, a.values, a.n_slots, ntiles, offsets, bytes, info, a.text,
                       a.text_stride, reinterpret_cast<long long*>(a.lengths), a.flags);
    DAD3D_HIP_TRY(hipGetLastError());
    return DAD3D_OK;
}

void json_number_host(const float* values, size_t n, unsigned char* out, size_t out_stride, int* lengths) {
    for (size_t i = 0; i < n; ++i) {
        unsigned bits;
        __builtin_memcpy(&bits, values + i, 4);
        JsonNumber num;
        if (!json_number(bits, num)) {
            lengths[i] = -1;
            continue;
        }
        unsigned char* end = json_put_number(out + i * out_stride, num);
        lengths[i] = (int)(end - (out + i * out_stride));
    }
}

}  // namespace dad3d
