// C ABI, files: .obj and JSON text, JSON and annotation parsing, the PNG, zlib and JPEG codecs. No handles: every call is stateless.
#include "capi_checks.hpp"

using namespace dad3d;

extern "C" {

size_t dad3d_obj_format_scratch_bytes(int batch, int nver) {
    return batch < 0 || nver < 0 ? 0 : obj_format_scratch_bytes(batch, nver);
}

dad3d_status dad3d_obj_format_vertices(const float* vertices, int batch, int nver, uint8_t* text, size_t text_stride, int64_t* lengths,
                                       int32_t* flags, void* scratch, size_t scratch_bytes, int device, void* stream) {
    DAD3D_REQUIRE(batch >= 0 && nver >= 0, "dad3d_obj_format_vertices: bad argument");
    DAD3D_REQUIRE(batch <= 65535 && nver <= 0x7fffffff / DAD3D_OBJ_MAX_LINE_BYTES, "dad3d_obj_format_vertices: batch %d / %d vertices beyond the launch grid",
                  batch, nver);
    if (batch == 0) return DAD3D_OK;
    DAD3D_REQUIRE((vertices || nver == 0) && text && lengths && flags && scratch, "dad3d_obj_format_vertices: null argument");
    DAD3D_REQUIRE(text_stride >= (size_t)nver * DAD3D_OBJ_MAX_LINE_BYTES, "dad3d_obj_format_vertices: text_stride %zu is below the worst case of %d vertices (%zu bytes)",
                  text_stride, nver, (size_t)nver * DAD3D_OBJ_MAX_LINE_BYTES);
    DAD3D_REQUIRE(text_stride % 16 == 0 && aligned(text, 16), "dad3d_obj_format_vertices: text and text_stride must be 16-byte aligned");
    DAD3D_REQUIRE(aligned(scratch, 8) && aligned(lengths, 8) && aligned(flags, 4), "dad3d_obj_format_vertices: lengths / flags / scratch are misaligned");
    DAD3D_REQUIRE(scratch_bytes >= obj_format_scratch_bytes(batch, nver), "dad3d_obj_format_vertices: %zu bytes of scratch, %zu needed", scratch_bytes,
                  obj_format_scratch_bytes(batch, nver));
    DAD3D_SELECT_DEVICE(device);
    ObjFormatArgs a{vertices, text, text_stride, lengths, flags, scratch, batch, nver};
    return launch_obj_format(a, static_cast<hipStream_t>(stream));
}

size_t dad3d_json_format_scratch_bytes(int batch, int n_slots) {
    return batch < 1 || n_slots < 1 ? 0 : json_format_scratch_bytes(batch, n_slots);
}

dad3d_status dad3d_json_format_values(const float* values, int batch, int n_slots, const void* literals, const int32_t* literal_offsets,
                                      uint8_t* text, size_t text_stride, int64_t* lengths, int32_t* flags, void* scratch,
                                      size_t scratch_bytes, int device, void* stream) {
    DAD3D_REQUIRE(batch > 0 && n_slots > 0, "dad3d_json_format_values: batch %d and n_slots %d must be positive", batch, n_slots);
    DAD3D_REQUIRE(batch <= 65535 && n_slots <= 0x7fffffff / (DAD3D_JSON_MAX_LITERAL_BYTES + DAD3D_JSON_MAX_NUMBER_BYTES) - 1,
                  "dad3d_json_format_values: batch %d / %d slots beyond the launch grid", batch, n_slots);
    DAD3D_REQUIRE(values && literals && literal_offsets && text && lengths && flags && scratch, "dad3d_json_format_values: null argument");
    DAD3D_REQUIRE(literal_offsets[0] == 0, "dad3d_json_format_values: literal_offsets must start at 0");
    for (int i = 0; i <= n_slots; ++i) {
        const long long len = (long long)literal_offsets[i + 1] - literal_offsets[i];
        DAD3D_REQUIRE(len >= 0 && len <= DAD3D_JSON_MAX_LITERAL_BYTES, "dad3d_json_format_values: literal %d is %lld bytes long (0 .. %d allowed)", i,
                      len, DAD3D_JSON_MAX_LITERAL_BYTES);
    }
    const size_t worst = (size_t)literal_offsets[n_slots + 1] + (size_t)n_slots * DAD3D_JSON_MAX_NUMBER_BYTES;
    DAD3D_REQUIRE(text_stride >= worst, "dad3d_json_format_values: text_stride %zu is below the worst case of the template (%zu bytes)", text_stride,
                  worst);
    DAD3D_REQUIRE(text_stride % 16 == 0 && aligned(text, 16), "dad3d_json_format_values: text and text_stride must be 16-byte aligned");
    DAD3D_REQUIRE(aligned(scratch, 8) && aligned(lengths, 8) && aligned(flags, 4) && aligned(literals, 4) && aligned(values, 4),
                  "dad3d_json_format_values: values / literals / lengths / flags / scratch are misaligned");
    DAD3D_REQUIRE(scratch_bytes >= json_format_scratch_bytes(batch, n_slots), "dad3d_json_format_values: %zu bytes of scratch, %zu needed", scratch_bytes,
                  json_format_scratch_bytes(batch, n_slots));
    DAD3D_SELECT_DEVICE(device);
    JsonFormatArgs a{values, literals, text, text_stride, lengths, flags, scratch, batch, n_slots};
    return launch_json_format(a, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_json_number_host(const float* values, size_t n, uint8_t* out, size_t out_stride, int32_t* lengths) {
    if (n == 0) return DAD3D_OK;
    DAD3D_REQUIRE(values && out && lengths, "dad3d_json_number_host: null argument");
    DAD3D_REQUIRE(out_stride >= DAD3D_JSON_MAX_NUMBER_BYTES, "dad3d_json_number_host: out_stride %zu is below the longest number (%d bytes)", out_stride,
                  DAD3D_JSON_MAX_NUMBER_BYTES);
    json_number_host(values, n, out, out_stride, lengths);
    return DAD3D_OK;
}

static bool png_shape_ok(int h, int w, int c) {
    return h >= 1 && w >= 1 && c >= 1 && c <= 4 && (long long)w * c < 0x7fffffffll && png_stream_bytes(h, w, c) < 0x80000000ll;
}

size_t dad3d_png_max_bytes(int h, int w, int c) { return png_shape_ok(h, w, c) ? png_max_bytes(h, w, c) : 0; }

size_t dad3d_png_scratch_bytes(int batch, int h, int w, int c) {
    return batch >= 1 && batch <= 65535 && png_shape_ok(h, w, c) ? png_scratch_bytes(batch, h, w, c) : 0;
}

size_t dad3d_zlib_max_bytes(int64_t n) { return n >= 1 && n < 0x80000000ll ? zlib_max_bytes(n) : 0; }

size_t dad3d_zlib_scratch_bytes(int batch, int64_t n) {
    return batch >= 1 && batch <= 65535 && n >= 1 && n < 0x80000000ll ? zlib_scratch_bytes(batch, n) : 0;
}

static dad3d_status deflate_checked(const char* who, DeflateArgs& a, size_t max_bytes, size_t need_scratch, size_t scratch_bytes, int device,
                                    void* stream) {
    DAD3D_REQUIRE_BATCH(who, a.batch);
    DAD3D_REQUIRE(a.data && a.out && a.lengths && a.flags && a.scratch, "%s: null argument", who);
    DAD3D_REQUIRE(a.out_stride >= max_bytes, "%s: out_stride %zu is below the worst case of the shape (%zu bytes)", who, a.out_stride, max_bytes);
    DAD3D_REQUIRE(a.out_stride % 16 == 0 && aligned(a.out, 16), "%s: out and out_stride must be 16-byte aligned", who);
    DAD3D_REQUIRE(aligned(a.scratch, 16) && aligned(a.lengths, 8) && aligned(a.flags, 4), "%s: lengths / flags / scratch are misaligned", who);
    DAD3D_REQUIRE(scratch_bytes >= need_scratch, "%s: %zu bytes of scratch, %zu needed", who, scratch_bytes, need_scratch);
    DAD3D_SELECT_DEVICE(device);
    return launch_deflate(a, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_png_encode(const uint8_t* images, int batch, int h, int w, int c, uint8_t* out, size_t out_stride, int64_t* lengths,
                              int32_t* flags, void* scratch, size_t scratch_bytes, int device, void* stream) {
    DAD3D_REQUIRE(c >= 1 && c <= 4, "dad3d_png_encode: %d channels (1 .. 4: grey, grey + alpha, RGB, RGBA)", c);
    DAD3D_REQUIRE(h >= 1 && w >= 1, "dad3d_png_encode: an image of %d x %d", h, w);
    DAD3D_REQUIRE(png_shape_ok(h, w, c), "dad3d_png_encode: the filtered stream of a %d x %d x %d image passes 2^31 bytes", h, w, c);
    DAD3D_REQUIRE_BATCH("dad3d_png_encode", batch);
    DeflateArgs a{images, out, out_stride, lengths, flags, scratch, 0, batch, 1, h, w, c};
    return deflate_checked("dad3d_png_encode", a, png_max_bytes(h, w, c), png_scratch_bytes(batch, h, w, c), scratch_bytes, device, stream);
}

dad3d_status dad3d_zlib_compress(const uint8_t* data, int batch, int64_t n, uint8_t* out, size_t out_stride, int64_t* lengths, int32_t* flags,
                                 void* scratch, size_t scratch_bytes, int device, void* stream) {
    DAD3D_REQUIRE(n >= 1 && n < 0x80000000ll, "dad3d_zlib_compress: a stream of %lld bytes (1 .. 2^31 - 1)", (long long)n);
    DAD3D_REQUIRE_BATCH("dad3d_zlib_compress", batch);
    DeflateArgs a{data, out, out_stride, lengths, flags, scratch, n, batch, 0, 0, 0, 0};
    return deflate_checked("dad3d_zlib_compress", a, zlib_max_bytes(n), zlib_scratch_bytes(batch, n), scratch_bytes, device, stream);
}

dad3d_status dad3d_deflate_tables_host(const uint32_t* ll_hist, const uint32_t* d_hist, uint8_t* ll_len, uint8_t* d_len, uint8_t* cl_len,
                                       uint16_t* ll_code, uint16_t* d_code, uint16_t* cl_code, uint8_t* header, int32_t* header_bits,
                                       uint32_t* dynamic_bits, uint32_t* fixed_bits) {
    DAD3D_REQUIRE(ll_hist && d_hist && ll_len && d_len && cl_len && ll_code && d_code && cl_code && header && header_bits && dynamic_bits && fixed_bits,
                  "dad3d_deflate_tables_host: null argument");
    unsigned long long total = 0;
    for (int i = 0; i < 286 + 30; ++i) {
        const uint32_t v = i < 286 ? ll_hist[i] : d_hist[i - 286];
        DAD3D_REQUIRE(v < (1u << 22), "dad3d_deflate_tables_host: a count of %u (below 2^22)", v);
        total += v;
    }
    DAD3D_REQUIRE(total < (1ull << 26), "dad3d_deflate_tables_host: %llu symbols in one block (below 2^26)", total);
    return deflate_tables_host(ll_hist, d_hist, ll_len, d_len, cl_len, ll_code, d_code, cl_code, header, header_bits, dynamic_bits, fixed_bits);
}

size_t dad3d_png_decode_scratch_bytes(int64_t* desc, int batch, int32_t* max_segments) {
    if (!desc || !max_segments || batch < 1 || batch > 65535) return 0;
    static_assert(sizeof(long long) == sizeof(int64_t), "descriptor rows");
    int most = 0;
    const size_t bytes = png_decode_layout(reinterpret_cast<long long*>(desc), batch, &most);
    *max_segments = most;
    return bytes;
}

dad3d_status dad3d_png_decode(const uint8_t* files, size_t files_bytes, const int64_t* desc, int batch, int max_segments, uint8_t* out,
                              size_t out_bytes, int32_t* flags, int32_t* info, void* scratch, size_t scratch_bytes, int force_general, int device,
                              void* stream) {
    DAD3D_REQUIRE_BATCH("dad3d_png_decode", batch);
    DAD3D_REQUIRE(files && desc && out && flags && info && scratch, "dad3d_png_decode: null argument");
    DAD3D_REQUIRE(max_segments >= 1 && max_segments <= (1 << 18), "dad3d_png_decode: max_segments %d outside 1 .. 2^18", max_segments);
    DAD3D_REQUIRE(aligned(scratch, 16) && aligned(desc, 8), "dad3d_png_decode: scratch must be 16-byte aligned, desc 8-byte aligned");
    DAD3D_REQUIRE(scratch_bytes >= (size_t)batch * 16, "dad3d_png_decode: %zu bytes of scratch for a batch of %d", scratch_bytes, batch);
    DAD3D_SELECT_DEVICE(device);
    PngDecodeArgs a{files, files_bytes, reinterpret_cast<const long long*>(desc), batch, max_segments, force_general ? 1 : 0, out, out_bytes,
                    flags, info, static_cast<unsigned char*>(scratch), scratch_bytes};
    return launch_png_decode(a, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_zlib_decompress(const uint8_t* streams, size_t streams_bytes, const int64_t* desc, int batch, uint8_t* out, size_t out_bytes,
                                   int64_t* lengths, int32_t* flags, int device, void* stream) {
    DAD3D_REQUIRE_BATCH("dad3d_zlib_decompress", batch);
    DAD3D_REQUIRE(streams && desc && out && lengths && flags, "dad3d_zlib_decompress: null argument");
    DAD3D_REQUIRE(aligned(out, 16) && aligned(desc, 8), "dad3d_zlib_decompress: out must be 16-byte aligned, desc 8-byte aligned");
    DAD3D_SELECT_DEVICE(device);
    ZlibDecompressArgs a{streams, streams_bytes, reinterpret_cast<const long long*>(desc), batch, out, out_bytes, lengths, flags};
    return launch_zlib_decompress(a, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_inflate_host(const uint8_t* const* ranges, const int64_t* range_bytes, int n_ranges, uint8_t* out, int64_t capacity,
                                int64_t* length, int32_t* flag) {
    DAD3D_REQUIRE(n_ranges >= 0 && (n_ranges == 0 || (ranges && range_bytes)) && length && flag && capacity >= 0 && (out || capacity == 0),
                  "dad3d_inflate_host: null or negative argument");
    for (int i = 0; i < n_ranges; ++i)
        DAD3D_REQUIRE(range_bytes[i] >= 0 && (ranges[i] || range_bytes[i] == 0), "dad3d_inflate_host: range %d of %lld bytes", i, (long long)range_bytes[i]);
    long long n = 0;
    *flag = inflate_host(ranges, reinterpret_cast<const long long*>(range_bytes), n_ranges, out, capacity, &n);
    *length = n;
    return DAD3D_OK;
}

size_t dad3d_jpeg_decode_scratch_bytes(int64_t* desc, int batch, int32_t* grid) {
    if (!desc || !grid || batch < 1 || batch > 65535) return 0;
    int dims[DAD3D_JPEG_DECODE_GRID_INTS] = {0, 0, 0};
    const size_t bytes = jpeg_decode_layout(reinterpret_cast<long long*>(desc), batch, dims);
    for (int i = 0; i < DAD3D_JPEG_DECODE_GRID_INTS; ++i) grid[i] = dims[i];
    return bytes;
}

dad3d_status dad3d_jpeg_decode(const uint8_t* files, size_t files_bytes, const int64_t* desc, int batch, const int32_t* grid, uint8_t* out,
                               size_t out_bytes, int32_t* flags, void* scratch, size_t scratch_bytes, int device, void* stream) {
    DAD3D_REQUIRE_BATCH("dad3d_jpeg_decode", batch);
    DAD3D_REQUIRE(files && desc && grid && out && flags && scratch, "dad3d_jpeg_decode: null argument");
    DAD3D_REQUIRE(grid[0] >= 1 && grid[0] <= (1 << 22) && grid[1] >= 1 && grid[1] <= (1 << 22) && grid[2] >= 1 && grid[2] <= (1 << 28),
                  "dad3d_jpeg_decode: a grid of %d segments, %d blocks, %d pixels (dad3d_jpeg_decode_scratch_bytes gives it)", grid[0], grid[1], grid[2]);
    DAD3D_REQUIRE((long long)batch * ((grid[0] + 62) / 64) + (batch + 63) / 64 <= 0x7fffffffll, "dad3d_jpeg_decode: %d files of up to %d segments pass the grid",
                  batch, grid[0]);
    DAD3D_REQUIRE(aligned(scratch, 16) && aligned(desc, 8), "dad3d_jpeg_decode: scratch must be 16-byte aligned, desc 8-byte aligned");
    DAD3D_REQUIRE(scratch_bytes >= (size_t)batch * jpeg_decode_state_bytes(), "dad3d_jpeg_decode: %zu bytes of scratch for a batch of %d", scratch_bytes,
                  batch);
    DAD3D_SELECT_DEVICE(device);
    JpegDecodeArgs a{files, files_bytes, reinterpret_cast<const long long*>(desc), batch, grid[0], grid[1], grid[2], out, out_bytes,
                     flags, static_cast<unsigned char*>(scratch), scratch_bytes};
    return launch_jpeg_decode(a, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_jpeg_decode_host(const uint8_t* file, int64_t size, int channels, uint8_t* out, int64_t out_bytes, int32_t* h, int32_t* w,
                                    int32_t* c, int32_t* flag) {
    DAD3D_REQUIRE(size >= 0 && (file || size == 0) && h && w && c && flag && out_bytes >= 0, "dad3d_jpeg_decode_host: null or negative argument");
    DAD3D_REQUIRE(channels == 0 || channels == 1 || channels == 3, "dad3d_jpeg_decode_host: %d channels (0 the file's own, 1, 3)", channels);
    int hh = 0, ww = 0, cc = 0;
    bool fits = true;
    *flag = jpeg_decode_host(file, size, channels, out, out_bytes, &hh, &ww, &cc, &fits);
    *h = hh, *w = ww, *c = cc;
    DAD3D_REQUIRE(fits, "dad3d_jpeg_decode_host: a %d x %d x %d image does not fit %lld bytes", hh, ww, cc, (long long)out_bytes);
    return DAD3D_OK;
}

size_t dad3d_jpeg_decode_sync_scratch_bytes(int64_t* desc, int batch, int32_t* grid, int piece_bytes) {
    if (!desc || !grid || batch < 1 || batch > 65535) return 0;
    int dims[DAD3D_JPEG_DECODE_SYNC_GRID_INTS] = {0, 0, 0, 0};
    const size_t bytes = jpeg_decode_sync_layout(reinterpret_cast<long long*>(desc), batch, dims, piece_bytes);
    for (int i = 0; i < DAD3D_JPEG_DECODE_SYNC_GRID_INTS; ++i) grid[i] = dims[i];
    return bytes;
}

dad3d_status dad3d_jpeg_decode_sync(const uint8_t* files, size_t files_bytes, const int64_t* desc, int batch, const int32_t* grid, int piece_bytes,
                                    uint8_t* out, size_t out_bytes, int32_t* flags, int32_t* info, void* scratch, size_t scratch_bytes, int device,
                                    void* stream) {
    DAD3D_REQUIRE(piece_bytes >= 16 && piece_bytes <= 256 && (piece_bytes & (piece_bytes - 1)) == 0,
                  "dad3d_jpeg_decode_sync: pieces of %d bytes (a power of two, 16 .. 256)", piece_bytes);
    DAD3D_REQUIRE_BATCH("dad3d_jpeg_decode_sync", batch);
    DAD3D_REQUIRE(files && desc && grid && out && flags && info && scratch, "dad3d_jpeg_decode_sync: null argument");
    DAD3D_REQUIRE(grid[0] >= 1 && grid[0] <= (1 << 22) && grid[1] >= 1 && grid[1] <= (1 << 22) && grid[2] >= 1 && grid[2] <= (1 << 28) && grid[3] >= 1 &&
                      grid[3] <= (1 << 19),
                  "dad3d_jpeg_decode_sync: a grid of %d segments, %d blocks, %d pixels, %d groups (dad3d_jpeg_decode_sync_scratch_bytes gives it)", grid[0],
                  grid[1], grid[2], grid[3]);
    DAD3D_REQUIRE((long long)batch * grid[0] <= 64ll * 0x7fffffffll, "dad3d_jpeg_decode_sync: %d files of up to %d segments pass the grid", batch,
                  grid[0]);
    DAD3D_REQUIRE(aligned(scratch, 16) && aligned(desc, 8), "dad3d_jpeg_decode_sync: scratch must be 16-byte aligned, desc 8-byte aligned");
    DAD3D_REQUIRE(scratch_bytes >= (size_t)batch * jpeg_decode_state_bytes(), "dad3d_jpeg_decode_sync: %zu bytes of scratch for a batch of %d",
                  scratch_bytes, batch);
    DAD3D_SELECT_DEVICE(device);
    JpegDecodeSyncArgs a{{files, files_bytes, reinterpret_cast<const long long*>(desc), batch, grid[0], grid[1], grid[2], out, out_bytes, flags,
                          static_cast<unsigned char*>(scratch), scratch_bytes},
                         piece_bytes, grid[3], info};
    return launch_jpeg_decode_sync(a, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_jpeg_decode_sync_host(const uint8_t* file, int64_t size, int channels, int piece_bytes, uint8_t* out, int64_t out_bytes, int32_t* h,
                                         int32_t* w, int32_t* c, int32_t* flag, int32_t* info) {
    DAD3D_REQUIRE(size >= 0 && (file || size == 0) && h && w && c && flag && info && out_bytes >= 0,
                  "dad3d_jpeg_decode_sync_host: null or negative argument");
    DAD3D_REQUIRE(channels == 0 || channels == 1 || channels == 3, "dad3d_jpeg_decode_sync_host: %d channels (0 the file's own, 1, 3)", channels);
    DAD3D_REQUIRE(piece_bytes >= 16 && piece_bytes <= 256 && (piece_bytes & (piece_bytes - 1)) == 0,
                  "dad3d_jpeg_decode_sync_host: pieces of %d bytes (a power of two, 16 .. 256)", piece_bytes);
    int hh = 0, ww = 0, cc = 0, what[4] = {0, 0, 0, 0};
    bool fits = true;
    *flag = jpeg_decode_host(file, size, channels, out, out_bytes, &hh, &ww, &cc, &fits, piece_bytes, what);
    *h = hh, *w = ww, *c = cc;
    for (int i = 0; i < 4; ++i) info[i] = what[i];
    DAD3D_REQUIRE(fits, "dad3d_jpeg_decode_sync_host: a %d x %d x %d image does not fit %lld bytes", hh, ww, cc, (long long)out_bytes);
    return DAD3D_OK;
}

size_t dad3d_jpeg_max_bytes(int h, int w, int c, int subsampling) { return jpeg_encode_max_bytes(h, w, c, subsampling); }

size_t dad3d_jpeg_encode_scratch_bytes(int batch, int h, int w, int c, int subsampling) {
    return jpeg_encode_scratch_bytes(batch, h, w, c, subsampling);
}

static dad3d_status jpeg_encode_options_ok(const char* who, int h, int w, int c, int quality, int subsampling, int restart_interval) {
    DAD3D_REQUIRE(c == 1 || c == 3, "%s: %d channels (1 grey, 3 RGB)", who, c);
    DAD3D_REQUIRE(h >= 1 && w >= 1 && h <= 65535 && w <= 65535, "%s: an image of %d x %d (1 .. 65535)", who, h, w);
    DAD3D_REQUIRE(quality >= 1 && quality <= 100, "%s: quality %d outside 1 .. 100", who, quality);
    DAD3D_REQUIRE(subsampling >= 0 && subsampling <= 2, "%s: subsampling %d (0 4:4:4, 1 4:2:2, 2 4:2:0)", who, subsampling);
    DAD3D_REQUIRE(restart_interval >= 0 && restart_interval <= 65535, "%s: a restart interval of %d MCUs (0 .. 65535)", who, restart_interval);
    DAD3D_REQUIRE(jpeg_encode_max_bytes(h, w, c, subsampling) != 0, "%s: an image of %d x %d x %d has more than 2^22 blocks", who, h, w, c);
    return DAD3D_OK;
}

dad3d_status dad3d_jpeg_encode(const uint8_t* images, int batch, int h, int w, int c, int quality, int subsampling, int restart_interval,
                               uint8_t* out, size_t out_stride, int64_t* lengths, int32_t* flags, void* scratch, size_t scratch_bytes,
                               int device, void* stream) {
    const char* who = "dad3d_jpeg_encode";
    DAD3D_REQUIRE(images && out && lengths && flags && scratch, "%s: null argument", who);
    DAD3D_REQUIRE_BATCH(who, batch);
    if (const dad3d_status st = jpeg_encode_options_ok(who, h, w, c, quality, subsampling, restart_interval)) return st;
    const size_t worst = jpeg_encode_max_bytes(h, w, c, subsampling), need = jpeg_encode_scratch_bytes(batch, h, w, c, subsampling);
    DAD3D_REQUIRE(out_stride >= worst, "%s: out_stride %zu is below the worst case of the shape (%zu bytes)", who, out_stride, worst);
    DAD3D_REQUIRE(out_stride % 16 == 0 && aligned(out, 16), "%s: out and out_stride must be 16-byte aligned", who);
    DAD3D_REQUIRE(aligned(scratch, 16) && aligned(lengths, 8) && aligned(flags, 4), "%s: lengths / flags / scratch are misaligned", who);
    DAD3D_REQUIRE(scratch_bytes >= need, "%s: %zu bytes of scratch, %zu needed", who, scratch_bytes, need);
    DAD3D_SELECT_DEVICE(device);
    JpegEncodeArgs a{images, batch, h, w, c, quality, subsampling, restart_interval, out, out_stride, lengths, flags, scratch};
    return launch_jpeg_encode(a, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_jpeg_encode_host(const uint8_t* image, int h, int w, int c, int quality, int subsampling, int restart_interval, uint8_t* out,
                                    int64_t capacity, int64_t* length, int32_t* flag) {
    const char* who = "dad3d_jpeg_encode_host";
    DAD3D_REQUIRE(image && out && length && flag, "%s: null argument", who);
    if (const dad3d_status st = jpeg_encode_options_ok(who, h, w, c, quality, subsampling, restart_interval)) return st;
    DAD3D_REQUIRE(capacity >= (int64_t)jpeg_encode_max_bytes(h, w, c, subsampling), "%s: %lld bytes for a file of up to %zu", who,
                  (long long)capacity, jpeg_encode_max_bytes(h, w, c, subsampling));
    long long n = 0;
    *flag = jpeg_encode_host(image, h, w, c, quality, subsampling, restart_interval, out, capacity, &n);
    *length = n;
    return DAD3D_OK;
}

size_t dad3d_json_parse_scratch_bytes(int64_t n_bytes) {
    return n_bytes < 1 || n_bytes > 0x7fffffffLL ? 0 : json_parse_scratch_bytes(n_bytes);
}

dad3d_status dad3d_json_parse_index(const uint8_t* text, int64_t n_bytes, void* scratch, size_t scratch_bytes, int32_t* counts, int device,
                                    void* stream) {
    DAD3D_REQUIRE(n_bytes > 0 && n_bytes <= 0x7fffffffLL, "dad3d_json_parse_index: n_bytes %lld must be in 1 .. 2^31 - 1", (long long)n_bytes);
    DAD3D_REQUIRE(text && scratch && counts, "dad3d_json_parse_index: null argument");
    DAD3D_REQUIRE(aligned(text, 16) && aligned(scratch, 16) && aligned(counts, 4), "dad3d_json_parse_index: text / scratch / counts are misaligned");
    DAD3D_REQUIRE(scratch_bytes >= json_parse_scratch_bytes(n_bytes), "dad3d_json_parse_index: %zu bytes of scratch, %zu needed", scratch_bytes,
                  json_parse_scratch_bytes(n_bytes));
    DAD3D_SELECT_DEVICE(device);
    return launch_json_parse_index(text, n_bytes, scratch, counts, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_json_parse_lists(const uint8_t* text, int64_t n_bytes, const void* scratch, size_t scratch_bytes, int32_t* tok_pos,
                                    int32_t* tok_brk, int64_t tok_cap, int32_t* brk_pos, int32_t* brk_key, int32_t* brk_nonnum, int32_t* brk_tok,
                                    int64_t brk_cap, int device, void* stream) {
    DAD3D_REQUIRE(n_bytes > 0 && n_bytes <= 0x7fffffffLL, "dad3d_json_parse_lists: n_bytes %lld must be in 1 .. 2^31 - 1", (long long)n_bytes);
    DAD3D_REQUIRE(tok_cap >= 0 && brk_cap >= 0, "dad3d_json_parse_lists: negative capacity");
    DAD3D_REQUIRE(text && scratch && (tok_cap == 0 || (tok_pos && tok_brk)) && (brk_cap == 0 || (brk_pos && brk_key && brk_nonnum && brk_tok)),
                  "dad3d_json_parse_lists: null argument");
    DAD3D_REQUIRE(aligned(scratch, 16) && aligned(tok_pos, 4) && aligned(tok_brk, 4) && aligned(brk_pos, 4) && aligned(brk_key, 4) &&
                      aligned(brk_nonnum, 4) && aligned(brk_tok, 4),
                  "dad3d_json_parse_lists: scratch / lists are misaligned");
    DAD3D_REQUIRE(scratch_bytes >= json_parse_scratch_bytes(n_bytes), "dad3d_json_parse_lists: %zu bytes of scratch, %zu needed", scratch_bytes,
                  json_parse_scratch_bytes(n_bytes));
    DAD3D_SELECT_DEVICE(device);
    JsonParseListsArgs a{scratch, tok_pos, tok_brk, brk_pos, brk_key, brk_nonnum, brk_tok, n_bytes, tok_cap, brk_cap};
    return launch_json_parse_lists(a, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_json_parse_check_arrays(const uint8_t* text, int64_t n_bytes, const int32_t* tok_pos, const int32_t* tok_brk, int64_t n_tokens,
                                           const int32_t* brk_pos, const int32_t* brk_key, const int32_t* brk_tok, int64_t n_brackets,
                                           const int32_t* arr_open, const int32_t* arr_close, int32_t* arr_rows, int64_t n_arrays, int device,
                                           void* stream) {
    DAD3D_REQUIRE(n_bytes > 0 && n_bytes <= 0x7fffffffLL, "dad3d_json_parse_check_arrays: n_bytes %lld must be in 1 .. 2^31 - 1", (long long)n_bytes);
    DAD3D_REQUIRE(n_tokens >= 0 && n_brackets >= 0 && n_arrays >= 0 && n_tokens <= n_bytes && n_brackets <= n_bytes && n_arrays <= n_brackets,
                  "dad3d_json_parse_check_arrays: %lld tokens / %lld brackets / %lld arrays do not fit a document of %lld bytes", (long long)n_tokens,
                  (long long)n_brackets, (long long)n_arrays, (long long)n_bytes);
    if (n_arrays == 0) return DAD3D_OK;
    DAD3D_REQUIRE(text && (n_tokens == 0 || (tok_pos && tok_brk)) && brk_pos && brk_key && brk_tok && arr_open && arr_close && arr_rows,
                  "dad3d_json_parse_check_arrays: null argument");
    DAD3D_REQUIRE(aligned(tok_pos, 4) && aligned(tok_brk, 4) && aligned(brk_pos, 4) && aligned(brk_key, 4) && aligned(brk_tok, 4) &&
                      aligned(arr_open, 4) && aligned(arr_close, 4) && aligned(arr_rows, 4),
                  "dad3d_json_parse_check_arrays: lists are misaligned");
    DAD3D_SELECT_DEVICE(device);
    JsonParseCheckArgs a{text, tok_pos, tok_brk, brk_pos, brk_key, brk_tok, arr_open, arr_close, arr_rows, n_bytes, n_tokens, n_brackets, n_arrays};
    return launch_json_parse_check_arrays(a, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_json_parse_extract(const uint8_t* text, int64_t n_bytes, const int32_t* tok_pos, int64_t n_tokens, const int32_t* records,
                                      int64_t n_records, int64_t n_values, double* values, uint8_t* is_int, int64_t values_cap, int device,
                                      void* stream) {
    DAD3D_REQUIRE(n_bytes > 0 && n_bytes <= 0x7fffffffLL, "dad3d_json_parse_extract: n_bytes %lld must be in 1 .. 2^31 - 1", (long long)n_bytes);
    DAD3D_REQUIRE(n_tokens >= 0 && n_records >= 0 && n_values >= 0 && n_tokens <= n_bytes && n_values <= n_tokens && n_records <= n_values,
                  "dad3d_json_parse_extract: %lld records / %lld values do not fit %lld tokens", (long long)n_records, (long long)n_values,
                  (long long)n_tokens);
    DAD3D_REQUIRE(values_cap >= n_values, "dad3d_json_parse_extract: room for %lld values, %lld needed", (long long)values_cap, (long long)n_values);
    if (n_values == 0) return DAD3D_OK;
    DAD3D_REQUIRE(n_records > 0, "dad3d_json_parse_extract: %lld values but no record", (long long)n_values);
    DAD3D_REQUIRE(text && tok_pos && records && values && is_int, "dad3d_json_parse_extract: null argument");
    DAD3D_REQUIRE(aligned(tok_pos, 4) && aligned(records, 4) && aligned(values, 8), "dad3d_json_parse_extract: lists / values are misaligned");
    DAD3D_SELECT_DEVICE(device);
    JsonParseExtractArgs a{text, tok_pos, records, values, is_int, n_bytes, n_tokens, n_records, n_values};
    return launch_json_parse_extract(a, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_json_parse_number_host(const uint8_t* text, const int64_t* starts, const int64_t* ends, size_t n, uint64_t* bits_out,
                                          uint8_t* is_int_out, uint32_t* flags_out) {
    if (n == 0) return DAD3D_OK;
    DAD3D_REQUIRE(text && starts && ends && bits_out && is_int_out && flags_out, "dad3d_json_parse_number_host: null argument");
    json_parse_number_host(text, reinterpret_cast<const long long*>(starts), reinterpret_cast<const long long*>(ends), n,
                           reinterpret_cast<unsigned long long*>(bits_out), is_int_out, flags_out);
    return DAD3D_OK;
}

dad3d_status dad3d_annotation_parse(const uint8_t* text, int64_t n_bytes, const int64_t* doc_offsets, const int64_t* doc_sizes, int batch, int n_verts,
                                    float* vertices, float* model_view, float* projection, int32_t* status, int device, void* stream) {
    DAD3D_REQUIRE(batch >= 0 && batch <= 65535, "dad3d_annotation_parse: batch %d outside 0 .. 65535", batch);
    DAD3D_REQUIRE(n_verts >= 1 && n_verts <= (1 << 24), "dad3d_annotation_parse: n_verts %d outside 1 .. 2^24", n_verts);
    DAD3D_REQUIRE(n_bytes >= 0 && n_bytes <= 0x7fffffffLL * 65535, "dad3d_annotation_parse: n_bytes %lld is negative or too large", (long long)n_bytes);
    if (batch == 0) return DAD3D_OK;
    DAD3D_REQUIRE(text && doc_offsets && doc_sizes && vertices && model_view && projection && status, "dad3d_annotation_parse: null argument");
    DAD3D_REQUIRE(aligned(text, 16) && aligned(doc_offsets, 8) && aligned(doc_sizes, 8) && aligned(vertices, 4) &&
                      aligned(model_view, 4) && aligned(projection, 4) && aligned(status, 4),
                  "dad3d_annotation_parse: text must be 16-byte aligned, the tables 8-byte, the outputs 4-byte aligned");
    DAD3D_SELECT_DEVICE(device);
    AnnotationParseArgs a{text, n_bytes, reinterpret_cast<const long long*>(doc_offsets), reinterpret_cast<const long long*>(doc_sizes), batch, n_verts,
                          vertices, model_view, projection, status};
    return launch_annotation_parse(a, static_cast<hipStream_t>(stream));
}

}  // extern "C"
