// C ABI, stateless tensor entry points: projection, preprocessing, CNN glue, heatmap points, boxes and tracks, losses, the scorer.
#include <cmath>

#include "capi_checks.hpp"

using namespace dad3d;

extern "C" {

dad3d_status dad3d_project_vertices(const float* vertices, const float* model_view, const float* projection,
                                    const float* frame, int batch, int nver, float* world_homo, float* xy,
                                    int32_t* xy_int, int device, void* stream) {
    DAD3D_REQUIRE(batch >= 0 && nver >= 0, "dad3d_project_vertices: bad argument");
    DAD3D_REQUIRE(batch <= 65535, "dad3d_project_vertices: batch %d beyond the launch grid", batch);
    if (batch == 0 || nver == 0) return DAD3D_OK;
    DAD3D_REQUIRE(vertices && model_view && projection && frame, "dad3d_project_vertices: null input");
    DAD3D_SELECT_DEVICE(device);
    return launch_project_vertices(vertices, model_view, projection, frame, batch, nver, world_homo, xy, xy_int,
                                   static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_gt_keypoints(const float* vertices, const float* model_view, const float* projection,
                                const int32_t* frames, int batch, int nver, const int32_t* index, const int32_t* corners,
                                const float* weights, int n_subset, int out_size, int resize_mode, float* full, float* subset_px,
                                float* subset_norm, uint8_t* presence, int device, void* stream) {
    DAD3D_REQUIRE(batch >= 0 && nver >= 0 && n_subset >= 0 && out_size > 0, "dad3d_gt_keypoints: bad argument");
    DAD3D_REQUIRE(resize_mode == DAD3D_RESIZE_LONGEST_MAX_SIZE || resize_mode == DAD3D_RESIZE_RESIZE,
                  "dad3d_gt_keypoints: unknown resize mode %d", resize_mode);
    DAD3D_REQUIRE(batch <= 65535, "dad3d_gt_keypoints: batch %d beyond the launch grid", batch);
    DAD3D_REQUIRE((long long)nver + n_subset <= 0x7fffff00LL, "dad3d_gt_keypoints: %d + %d points beyond the launch grid", nver,
                  n_subset);
    DAD3D_REQUIRE(n_subset == 0 || ((index != nullptr) != (corners != nullptr) && (corners == nullptr) == (weights == nullptr)),
                  "dad3d_gt_keypoints: give either index or corners + weights for the subset");
    if (batch == 0 || nver + n_subset == 0) return DAD3D_OK;
    DAD3D_REQUIRE(vertices && model_view && projection && frames, "dad3d_gt_keypoints: null input");
    DAD3D_REQUIRE((nver == 0 || full) && (n_subset == 0 || (subset_px && subset_norm && presence)), "dad3d_gt_keypoints: null output");
    DAD3D_SELECT_DEVICE(device);
    GtKeypointsArgs a{vertices, model_view, projection, frames, index, corners, weights, full, subset_px, subset_norm, presence,
                      nver, n_subset, out_size, resize_mode};
    return launch_gt_keypoints(a, batch, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_preprocess_images(const int64_t* descs, int batch, int out_size, const float* mean, const float* std,
                                     float* out, int device, void* stream) {
    DAD3D_REQUIRE(batch >= 0 && out_size > 0, "dad3d_preprocess_images: bad argument");
    if (batch == 0) return DAD3D_OK;
    DAD3D_REQUIRE(descs && mean && std && out, "dad3d_preprocess_images: null argument");
    DAD3D_REQUIRE(batch <= 65535 && out_size <= 65535, "dad3d_preprocess_images: batch / size beyond the launch grid");
    DAD3D_SELECT_DEVICE(device);
    return launch_preprocess(reinterpret_cast<const long long*>(descs), batch, out_size, mean, std, out,
                             static_cast<hipStream_t>(stream));
}

static int dtype_vec(int dtype) { return dtype == DAD3D_DTYPE_F32 ? 4 : (dtype == DAD3D_DTYPE_F16 || dtype == DAD3D_DTYPE_BF16) ? 8 : 0; }

dad3d_status dad3d_nhwc_bias_act(void* y, const void* bias, const void* z, int64_t n_pixels, int channels, int dtype, int relu,
                                 int device, void* stream) {
    DAD3D_REQUIRE(n_pixels >= 0 && channels > 0 && dtype_vec(dtype), "dad3d_nhwc_bias_act: bad argument");
    if (n_pixels == 0) return DAD3D_OK;
    DAD3D_REQUIRE(y && bias, "dad3d_nhwc_bias_act: null tensor");
    DAD3D_REQUIRE(channels % dtype_vec(dtype) == 0, "dad3d_nhwc_bias_act: %d channels are not a multiple of %d (16 bytes)", channels, dtype_vec(dtype));
    DAD3D_REQUIRE(aligned(y, 16) && aligned(bias, 16) && aligned(z, 16), "dad3d_nhwc_bias_act: tensors must be 16-byte aligned");
    DAD3D_SELECT_DEVICE(device);
    return launch_nhwc_bias_act(y, bias, z, (size_t)n_pixels, channels, dtype, relu, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_nhwc_resize_sum(void* out, int n, int oh, int ow, int channels, int dtype, int n_inputs, const void* const* xs,
                                   const int* hs, const int* ws, const float* weights, int device, void* stream) {
    DAD3D_REQUIRE(n >= 0 && oh >= 0 && ow >= 0 && channels > 0 && dtype_vec(dtype) && n_inputs >= 1 && n_inputs <= 3,
                  "dad3d_nhwc_resize_sum: bad argument");
    if (n == 0 || oh == 0 || ow == 0) return DAD3D_OK;
    DAD3D_REQUIRE(out && xs && hs && ws && weights, "dad3d_nhwc_resize_sum: null argument");
    DAD3D_REQUIRE(channels % dtype_vec(dtype) == 0, "dad3d_nhwc_resize_sum: %d channels are not a multiple of %d (16 bytes)", channels, dtype_vec(dtype));
    DAD3D_REQUIRE(aligned(out, 16), "dad3d_nhwc_resize_sum: tensors must be 16-byte aligned");
    for (int j = 0; j < n_inputs; ++j)
        DAD3D_REQUIRE(xs[j] && hs[j] > 0 && ws[j] > 0 && aligned(xs[j], 16),
                      "dad3d_nhwc_resize_sum: input %d is null, empty or not 16-byte aligned", j);
    DAD3D_SELECT_DEVICE(device);
    return launch_nhwc_resize_sum(out, n, oh, ow, channels, dtype, n_inputs, xs, hs, ws, weights, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_nhwc_fusion_concat(void* out, const void* x, const void* heat, const void* level, int n, int oh, int ow, int hh, int hw,
                                      int cx, int ch, int cl, int dtype, int device, void* stream) {
    DAD3D_REQUIRE(n >= 0 && oh >= 0 && ow >= 0 && hh > 0 && hw > 0 && cx > 0 && ch > 0 && cl > 0 && dtype_vec(dtype),
                  "dad3d_nhwc_fusion_concat: bad argument");
    const int per_piece = dtype_vec(dtype) / 2;  // elements of 8 bytes
    DAD3D_REQUIRE(cx % per_piece == 0 && ch % per_piece == 0 && cl % per_piece == 0,
                  "dad3d_nhwc_fusion_concat: %d / %d / %d channels are not multiples of %d (8 bytes)", cx, ch, cl, per_piece);
    DAD3D_REQUIRE((int64_t)cx + ch + cl <= 0x7fffffff && (int64_t)n * hh * hw <= 0x7fffffff && (int64_t)n * oh * ow <= 0x7fffffff,
                  "dad3d_nhwc_fusion_concat: sizes beyond 2^31 - 1");
    if (n == 0 || oh == 0 || ow == 0) return DAD3D_OK;
    DAD3D_REQUIRE(out && x && heat && level, "dad3d_nhwc_fusion_concat: null tensor");
    DAD3D_REQUIRE(aligned(out, 16) && aligned(x, 16) && aligned(heat, 16) && aligned(level, 16),
                  "dad3d_nhwc_fusion_concat: tensors must be 16-byte aligned");
    DAD3D_SELECT_DEVICE(device);
    return launch_nhwc_fusion_concat(out, x, heat, level, n, oh, ow, hh, hw, cx, ch, cl, dtype, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_nhwc_bias_mul(void* y, const void* bias, const void* x, int64_t n_pixels, int channels, int dtype, int device, void* stream) {
    DAD3D_REQUIRE(n_pixels >= 0 && channels > 0 && dtype_vec(dtype), "dad3d_nhwc_bias_mul: bad argument");
    if (n_pixels == 0) return DAD3D_OK;
    DAD3D_REQUIRE(y && bias && x, "dad3d_nhwc_bias_mul: null tensor");
    DAD3D_REQUIRE(channels % dtype_vec(dtype) == 0, "dad3d_nhwc_bias_mul: %d channels are not a multiple of %d (16 bytes)", channels, dtype_vec(dtype));
    DAD3D_REQUIRE(aligned(y, 16) && aligned(bias, 16) && aligned(x, 16), "dad3d_nhwc_bias_mul: tensors must be 16-byte aligned");
    DAD3D_SELECT_DEVICE(device);
    return launch_nhwc_bias_mul(y, bias, x, (size_t)n_pixels, channels, dtype, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_regression_heads(const void* top, int batch, int channels, int hw, int dtype, const dad3d_head_desc* heads, int n_heads,
                                    float* workspace, float* pooled_out, float* hidden_out, int device, void* stream) {
    const int vec = dtype_vec(dtype);
    DAD3D_REQUIRE(vec, "dad3d_regression_heads: unknown dtype %d", dtype);
    DAD3D_REQUIRE(batch > 0 && batch <= 65535 && channels > 0 && hw > 0 && n_heads >= 1 && n_heads <= DAD3D_HEADS_MAX,
                  "dad3d_regression_heads: bad size (batch %d, channels %d, hw %d, heads %d)", batch, channels, hw, n_heads);
    DAD3D_REQUIRE(channels % vec == 0, "dad3d_regression_heads: %d channels are not a multiple of %d (16 bytes)", channels, vec);
    DAD3D_REQUIRE((int64_t)hw * (channels / vec) <= 0x7fffffff, "dad3d_regression_heads: an image of %d x %d is beyond 2^31 - 1 vectors", hw, channels);
    DAD3D_REQUIRE(top && heads && workspace, "dad3d_regression_heads: null argument");
    DAD3D_REQUIRE(aligned(top, 16) && aligned(workspace, 16) && aligned(pooled_out, 16) && aligned(hidden_out, 16),
                  "dad3d_regression_heads: tensors must be 16-byte aligned");
    RegressionHeadsArgs a{top, batch, channels, hw, dtype, n_heads, {}, nullptr, nullptr};
    for (int j = 0; j < n_heads; ++j) {
        const dad3d_head_desc& d = heads[j];
        DAD3D_REQUIRE(d.hidden > 0 && d.out_dim > 0 && d.hidden % vec == 0, "dad3d_regression_heads: head %d: hidden %d (a multiple of %d), out_dim %d", j,
                      d.hidden, vec, d.out_dim);
        DAD3D_REQUIRE(d.act >= DAD3D_HEAD_ACT_NONE && d.act <= DAD3D_HEAD_ACT_TANH, "dad3d_regression_heads: head %d: unknown activation %d", j, d.act);
        DAD3D_REQUIRE(d.w1 && d.b1 && d.w2 && d.b2 && d.dst, "dad3d_regression_heads: head %d: null tensor", j);
        DAD3D_REQUIRE(aligned(d.w1, 16) && aligned(d.w2, 16) && aligned(d.b1, vec == 4 ? 4 : 2) && aligned(d.b2, vec == 4 ? 4 : 2) && aligned(d.dst, 4),
                      "dad3d_regression_heads: head %d: misaligned tensor", j);
        DAD3D_REQUIRE(d.dst_col_offset >= 0 && d.dst_row_stride >= d.dst_col_offset + d.out_dim,
                      "dad3d_regression_heads: head %d: a destination row of %lld floats does not hold columns %lld .. +%d", j,
                      (long long)d.dst_row_stride, (long long)d.dst_col_offset, d.out_dim);
        a.head[j] = d;
    }
    a.pooled = pooled_out ? pooled_out : workspace;
    a.hidden = hidden_out ? hidden_out : workspace + (size_t)batch * channels;
    DAD3D_SELECT_DEVICE(device);
    return launch_regression_heads(a, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_heatmap_argmax(const void* heatmap, int dtype, int batch, int channels, int h, int w, int layout, int sigmoid,
                                  int32_t* yx_out, float* peak_out, int device, void* stream) {
    const int es = dtype == DAD3D_DTYPE_F32 ? 4 : (dtype == DAD3D_DTYPE_F16 || dtype == DAD3D_DTYPE_BF16) ? 2 : dtype == DAD3D_HEATMAP_DTYPE_U8 ? 1 : 0;
    DAD3D_REQUIRE(es, "dad3d_heatmap_argmax: unknown dtype %d", dtype);
    DAD3D_REQUIRE(layout == DAD3D_LAYOUT_NCHW || layout == DAD3D_LAYOUT_NHWC, "dad3d_heatmap_argmax: unknown layout %d", layout);
    DAD3D_REQUIRE(batch > 0 && channels > 0 && h > 0 && w > 0, "dad3d_heatmap_argmax: bad size (batch %d, channels %d, h %d, w %d)", batch,
                  channels, h, w);
    DAD3D_REQUIRE((int64_t)h * w <= (1 << 24), "dad3d_heatmap_argmax: a plane of %d x %d is beyond 2^24 positions", h, w);
    DAD3D_REQUIRE((int64_t)batch * channels <= 0x7fffffff, "dad3d_heatmap_argmax: %d x %d planes are beyond the launch grid", batch, channels);
    DAD3D_REQUIRE(!(sigmoid && dtype == DAD3D_HEATMAP_DTYPE_U8), "dad3d_heatmap_argmax: no sigmoid of a uint8 heatmap");
    DAD3D_REQUIRE(heatmap && yx_out, "dad3d_heatmap_argmax: null argument");
    DAD3D_REQUIRE(aligned(heatmap, es), "dad3d_heatmap_argmax: the heatmap is not aligned to its %d-byte elements", es);
    DAD3D_SELECT_DEVICE(device);
    HeatmapArgmaxArgs a{heatmap, dtype, batch, channels, h, w, layout, sigmoid != 0, yx_out, peak_out, 1};
    return launch_heatmap_argmax(a, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_points_readjust(const void* src, int src_kind, int batch, int n_points, float mul, float limit, const double* geometry,
                                   int pad_left, int pad_top, double scale, int32_t* points_out, int device, void* stream) {
    DAD3D_REQUIRE(src_kind == DAD3D_POINTS_SRC_XY_F32 || src_kind == DAD3D_POINTS_SRC_YX_I32, "dad3d_points_readjust: unknown src_kind %d", src_kind);
    DAD3D_REQUIRE(batch > 0 && n_points > 0, "dad3d_points_readjust: bad size (batch %d, n_points %d)", batch, n_points);
    DAD3D_REQUIRE((int64_t)batch * n_points * 2 <= 0x7fffffff, "dad3d_points_readjust: %d x %d points are beyond the launch grid", batch, n_points);
    DAD3D_REQUIRE(src && points_out, "dad3d_points_readjust: null argument");
    DAD3D_REQUIRE(geometry || (scale > 0.0 && scale <= 1.7976931348623157e308), "dad3d_points_readjust: the scale must be a positive finite number");
    DAD3D_SELECT_DEVICE(device);
    PointsReadjustArgs a{src, src_kind, batch, n_points, mul, limit, geometry, pad_left, pad_top, scale, points_out};
    return launch_points_readjust(a, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_preprocess_boxes(const int64_t* images, int n_images, const void* boxes, int box_dtype, const int32_t* image_index,
                                    int n_boxes, const double* offset, int out_size, const float* mean, const float* std, int out_format,
                                    void* out, int32_t* crops, double* geometry, int32_t* flags, int device, void* stream) {
    DAD3D_REQUIRE(n_boxes >= 0 && n_boxes <= 65535 && out_size >= 1 && out_size <= 65535,
                  "dad3d_preprocess_boxes: %d boxes / size %d outside the launch grid (65535)", n_boxes, out_size);
    DAD3D_REQUIRE(box_dtype >= DAD3D_BOX_DTYPE_I32 && box_dtype <= DAD3D_BOX_DTYPE_F64, "dad3d_preprocess_boxes: unknown box_dtype %d", box_dtype);
    DAD3D_REQUIRE(out_format >= DAD3D_PREPROCESS_OUT_F32_NCHW && out_format <= DAD3D_PREPROCESS_OUT_BF16_NHWC,
                  "dad3d_preprocess_boxes: unknown out_format %d", out_format);
    if (n_boxes == 0) return DAD3D_OK;
    DAD3D_REQUIRE(n_images >= 1 && n_images <= 65535, "dad3d_preprocess_boxes: %d images outside 1 .. 65535", n_images);
    DAD3D_REQUIRE(images && boxes && image_index && mean && std && out && crops && geometry && flags, "dad3d_preprocess_boxes: null argument");
    DAD3D_REQUIRE(aligned(out, 4), "dad3d_preprocess_boxes: out must be 4-byte aligned");
    PreprocessBoxesArgs a{};
    if (offset) {
        for (int k = 0; k < 4; ++k)
            DAD3D_REQUIRE(offset[k] - offset[k] == 0.0, "dad3d_preprocess_boxes: offset[%d] is not finite", k);
        a.has_offset = 1, a.left = offset[0], a.right = offset[1], a.top = offset[2], a.bottom = offset[3];
    }
    DAD3D_SELECT_DEVICE(device);
    a.images = reinterpret_cast<const long long*>(images), a.n_images = n_images;
    a.boxes = boxes, a.box_dtype = box_dtype, a.image_index = image_index, a.n_boxes = n_boxes;
    a.out_size = out_size, a.out_format = out_format, a.out = out, a.crops = crops, a.geometry = geometry, a.flags = flags;
    return launch_preprocess_boxes(a, mean, std, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_points_readjust_frame(const void* src, int src_kind, int batch, int n_points, float mul, float limit, const double* geometry,
                                         int32_t* points_out, int device, void* stream) {
    DAD3D_REQUIRE(src_kind == DAD3D_POINTS_SRC_XY_F32 || src_kind == DAD3D_POINTS_SRC_YX_I32, "dad3d_points_readjust_frame: unknown src_kind %d", src_kind);
    DAD3D_REQUIRE(batch > 0 && n_points > 0, "dad3d_points_readjust_frame: bad size (batch %d, n_points %d)", batch, n_points);
    DAD3D_REQUIRE((int64_t)batch * n_points * 2 <= 0x7fffffff, "dad3d_points_readjust_frame: %d x %d points are beyond the launch grid", batch, n_points);
    DAD3D_REQUIRE(src && points_out && geometry, "dad3d_points_readjust_frame: null argument");
    DAD3D_SELECT_DEVICE(device);
    PointsReadjustArgs a{src, src_kind, batch, n_points, mul, limit, geometry, 0, 0, 1.0, points_out};
    return launch_points_readjust_frame(a, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_boxes_from_heads(const float* proj, int n_heads, int n_verts, int64_t head_stride, int vertex_stride, const int32_t* subset,
                                    int n_subset, const int64_t* frames, int n_frames, const int32_t* image_index, const int32_t* prev_flags,
                                    int min_side, double min_visible, int32_t* boxes, int32_t* flags, int device, void* stream) {
    DAD3D_REQUIRE(n_heads >= 0 && n_heads <= 65535, "dad3d_boxes_from_heads: %d heads outside the launch grid (65535)", n_heads);
    DAD3D_REQUIRE(n_verts >= 1 && n_verts <= 65535, "dad3d_boxes_from_heads: %d vertices outside 1 .. 65535", n_verts);
    DAD3D_REQUIRE(vertex_stride >= 2, "dad3d_boxes_from_heads: a vertex stride of %d floats holds no (x, y)", vertex_stride);
    DAD3D_REQUIRE((subset == nullptr) == (n_subset == 0), "dad3d_boxes_from_heads: a subset and its count go together (NULL and 0 for all vertices)");
    DAD3D_REQUIRE(n_subset >= 0 && n_subset <= 65535, "dad3d_boxes_from_heads: %d subset indices outside 1 .. 65535", n_subset);
    DAD3D_REQUIRE(min_side >= 0, "dad3d_boxes_from_heads: min_side %d is negative", min_side);
    DAD3D_REQUIRE(min_visible >= 0.0 && min_visible <= 1.0, "dad3d_boxes_from_heads: min_visible %g is outside [0, 1]", min_visible);  // false for a NaN
    if (n_heads == 0) return DAD3D_OK;
    DAD3D_REQUIRE(n_frames >= 1 && n_frames <= 65535, "dad3d_boxes_from_heads: %d frames outside 1 .. 65535", n_frames);
    DAD3D_REQUIRE(proj && frames && image_index && boxes && flags, "dad3d_boxes_from_heads: null argument");
    DAD3D_SELECT_DEVICE(device);
    TrackBoxesArgs a{proj, n_heads, n_verts, (long long)head_stride, vertex_stride, subset, n_subset, reinterpret_cast<const long long*>(frames),
                     n_frames, image_index, prev_flags, min_side, min_visible, boxes, flags};
    return launch_boxes_from_heads(a, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_one_euro_rows(const float* x, int64_t x_stride, float* out, int64_t out_stride, int n, int d, const int32_t* flags,
                                 const float* min_cutoff, const float* beta, float rate, float two_pi_dt, float alpha_d, float* state_x,
                                 float* state_dx, int32_t* age, int device, void* stream) {
    DAD3D_REQUIRE(d >= 1 && n >= 0, "dad3d_one_euro_rows: bad size (n %d, d %d)", n, d);
    DAD3D_REQUIRE(x_stride >= d && out_stride >= d, "dad3d_one_euro_rows: a row stride (%lld, %lld) is below d = %d", (long long)x_stride,
                  (long long)out_stride, d);
    for (float v : {rate, two_pi_dt, alpha_d})  // false for a NaN
        DAD3D_REQUIRE(v > 0.0f && v - v == 0.0f, "dad3d_one_euro_rows: the scalar %g is not finite and positive", (double)v);
    DAD3D_REQUIRE(alpha_d <= 1.0f, "dad3d_one_euro_rows: alpha_d %g is above 1", (double)alpha_d);
    if (n == 0) return DAD3D_OK;
    DAD3D_REQUIRE(x && out && min_cutoff && beta && state_x && state_dx && age, "dad3d_one_euro_rows: null argument");
    DAD3D_SELECT_DEVICE(device);
    OneEuroArgs a{x, (long long)x_stride, out, (long long)out_stride, n, d, flags, min_cutoff, beta, rate, two_pi_dt, alpha_d, state_x, state_dx, age};
    return launch_one_euro_rows(a, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_track_suppress_duplicates(int32_t* boxes, int32_t* flags, const int32_t* image_index, int n, double merge_iou, int device,
                                             void* stream) {
    DAD3D_REQUIRE(merge_iou > 0.0 && merge_iou <= 1.0, "dad3d_track_suppress_duplicates: merge_iou %g is outside (0, 1]", merge_iou);  // false for a NaN
    DAD3D_REQUIRE(n >= 0 && n <= DAD3D_TRACK_MAX_SLOTS, "dad3d_track_suppress_duplicates: %d slots outside 0 .. %d", n, DAD3D_TRACK_MAX_SLOTS);
    if (n == 0) return DAD3D_OK;
    DAD3D_REQUIRE(boxes && flags && image_index, "dad3d_track_suppress_duplicates: null argument");
    DAD3D_SELECT_DEVICE(device);
    SuppressDuplicatesArgs a{boxes, flags, image_index, n, merge_iou};
    return launch_suppress_duplicates(a, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_track_assign_detections(int32_t* boxes, int32_t* flags, int32_t* image_index, int32_t* misses, int n, const int32_t* det_boxes,
                                           const int32_t* det_index, const int32_t* det_count, int m, const int32_t* frame_searched, int n_frames,
                                           double match_iou, int refresh, int max_misses, int32_t* assign, int32_t* det_flags, int32_t* spawned,
                                           int device, void* stream) {
    const char* who = "dad3d_track_assign_detections";
    DAD3D_REQUIRE(match_iou > 0.0 && match_iou <= 1.0, "%s: match_iou %g is outside (0, 1]", who, match_iou);  // false for a NaN
    DAD3D_REQUIRE(n >= 0 && n <= DAD3D_TRACK_MAX_SLOTS, "%s: %d slots outside 0 .. %d", who, n, DAD3D_TRACK_MAX_SLOTS);
    DAD3D_REQUIRE(m >= 0 && m <= DAD3D_TRACK_MAX_DETECTIONS, "%s: %d detections outside 0 .. %d", who, m, DAD3D_TRACK_MAX_DETECTIONS);
    DAD3D_REQUIRE(n_frames >= 1, "%s: %d frames", who, n_frames);
    DAD3D_REQUIRE(refresh == 0 || refresh == 1, "%s: refresh %d is neither 0 nor 1", who, refresh);
    DAD3D_REQUIRE(max_misses < 0 || misses || n == 0, "%s: max_misses %d needs the misses it counts", who, max_misses);
    DAD3D_REQUIRE(n == 0 || (boxes && flags && image_index && spawned), "%s: null slot argument", who);
    DAD3D_REQUIRE(m == 0 || (det_boxes && det_index && assign && det_flags), "%s: null detection argument", who);
    if (n == 0 && m == 0) return DAD3D_OK;
    DAD3D_SELECT_DEVICE(device);
    AssignDetectionsArgs a{boxes, flags, image_index, misses, n, det_boxes, det_index, det_count, m, frame_searched, n_frames, match_iou,
                           refresh, max_misses, assign, det_flags, spawned};
    return launch_assign_detections(a, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_cube_region_loss(const float* pred, const float* target, int batch, int n_verts,
                                    const int32_t* region_ptr, const int32_t* region_idx, const float* region_weight,
                                    int n_regions, const int32_t* vert_ptr, const int32_t* vert_region,
                                    const int32_t* vert_pos, int criterion, float* stats, float* loss_terms,
                                    float* grad_pred, int device, void* stream) {
    DAD3D_REQUIRE(batch >= 0 && n_verts >= 0 && n_regions >= 0, "dad3d_cube_region_loss: negative size");
    DAD3D_REQUIRE(criterion >= DAD3D_LOSS_L1 && criterion <= DAD3D_LOSS_SMOOTH_L1, "dad3d_cube_region_loss: unknown criterion %d", criterion);
    if (batch == 0 || n_regions == 0) return DAD3D_OK;
    DAD3D_REQUIRE(pred && target && region_ptr && region_idx && region_weight && stats && loss_terms,
                  "dad3d_cube_region_loss: null argument");
    DAD3D_REQUIRE(!grad_pred || (vert_ptr && vert_region && vert_pos), "dad3d_cube_region_loss: the gradient needs the vertex incidence list");
    DAD3D_REQUIRE(batch <= 65535 && n_regions <= 65535, "dad3d_cube_region_loss: batch / regions beyond the launch grid");
    DAD3D_SELECT_DEVICE(device);
    CubeLossArgs a{pred, target, region_ptr, region_idx, region_weight, vert_ptr, vert_region, vert_pos, stats, loss_terms,
                   grad_pred, batch, n_verts, n_regions, criterion};
    return launch_cube_loss(a, static_cast<hipStream_t>(stream));
}

int dad3d_point_loss_terms(int n_points) { return point_loss_blocks(n_points); }

dad3d_status dad3d_weighted_point_loss(const float* pred, const float* target, int batch, int n_points, int comps,
                                       const float* point_weight, float scale, int criterion, float* loss_terms,
                                       float* grad_pred, int device, void* stream) {
    DAD3D_REQUIRE(batch >= 0 && n_points >= 0 && comps > 0, "dad3d_weighted_point_loss: bad size");
    DAD3D_REQUIRE(criterion >= DAD3D_LOSS_L1 && criterion <= DAD3D_LOSS_SMOOTH_L1, "dad3d_weighted_point_loss: unknown criterion %d", criterion);
    if (batch == 0 || n_points == 0) return DAD3D_OK;
    DAD3D_REQUIRE(pred && target && point_weight && loss_terms, "dad3d_weighted_point_loss: null argument");
    DAD3D_REQUIRE(batch <= 65535, "dad3d_weighted_point_loss: batch beyond the launch grid");
    DAD3D_SELECT_DEVICE(device);
    PointLossArgs a{pred, target, point_weight, loss_terms, grad_pred, scale, batch, n_points, comps, criterion};
    return launch_point_loss(a, static_cast<hipStream_t>(stream));
}

// ---- the rest of the training objective (train_objective.hip) ----------------------------------------------------------
dad3d_status dad3d_heatmap_encode(void* out, int form, const float* keypoints, const uint8_t* presence, int batch,
                                  int n_classes, float stride, int size, int radius, const void* table, int32_t* invalid,
                                  int device, void* stream) {
    DAD3D_REQUIRE(form >= DAD3D_HEATMAP_RAW && form <= DAD3D_HEATMAP_FLOAT, "dad3d_heatmap_encode: unknown form %d", form);
    DAD3D_REQUIRE(batch >= 0 && n_classes >= 0 && size >= 0, "dad3d_heatmap_encode: negative size");
    DAD3D_REQUIRE(size <= 46340, "dad3d_heatmap_encode: heatmap size %d beyond 46340", size);
    DAD3D_REQUIRE(radius >= 0 && radius <= 4096, "dad3d_heatmap_encode: radius %d outside 0..4096", radius);
    DAD3D_REQUIRE(std::isfinite(stride) && stride > 0.0f, "dad3d_heatmap_encode: stride must be finite and positive");
    if (batch == 0 || n_classes == 0 || size == 0) return DAD3D_OK;
    DAD3D_REQUIRE(out && keypoints && presence && table, "dad3d_heatmap_encode: null argument");
    DAD3D_REQUIRE(aligned(out, 16), "dad3d_heatmap_encode: the output must be 16-byte aligned");
    DAD3D_SELECT_DEVICE(device);
    HeatmapEncodeArgs a{out, keypoints, presence, table, invalid, (size_t)batch * n_classes, stride, size, radius, form};
    return launch_heatmap_encode(a, static_cast<hipStream_t>(stream));
}

static dad3d_status iou_check(const char* who, const float* pred, const void* target, int target_u8, int batch, int channels,
                              int hw) {
    DAD3D_REQUIRE(batch >= 0 && channels >= 0 && hw >= 0, "%s: negative size", who);
    DAD3D_REQUIRE(target_u8 == 0 || target_u8 == 1, "%s: target_u8 must be 0 or 1", who);
    DAD3D_REQUIRE((long long)batch * channels <= 0x7fffffffLL, "%s: %d x %d channels beyond the launch grid", who, batch, channels);
    DAD3D_REQUIRE(batch == 0 || channels == 0 || (pred && target), "%s: null argument", who);
    return DAD3D_OK;
}

static bool iou_vec(const float* pred, const void* target, int target_u8, int hw) {
    return hw % 4 == 0 && aligned(pred, 16) && aligned(target, target_u8 ? 4 : 16);
}

dad3d_status dad3d_heatmap_iou(const float* pred, const void* target, int target_u8, int batch, int channels, int hw,
                               int sigmoid, double* sums, float* iou, float* loss, float* accum, int device, void* stream) {
    dad3d_status st = iou_check("dad3d_heatmap_iou", pred, target, target_u8, batch, channels, hw);
    if (st) return st;
    DAD3D_REQUIRE(batch > 0 && channels > 0, "dad3d_heatmap_iou: no channels (the reference's mean over none is NaN)");
    DAD3D_REQUIRE(sums, "dad3d_heatmap_iou: null sums");
    DAD3D_REQUIRE(!accum || loss, "dad3d_heatmap_iou: accum needs loss");
    DAD3D_SELECT_DEVICE(device);
    IouArgs a{pred, target, sums, iou, loss, accum, nullptr, nullptr, (size_t)batch * channels, hw, target_u8 != 0};
    return launch_heatmap_iou(a, sigmoid != 0, iou_vec(pred, target, target_u8, hw), static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_heatmap_iou_grad(const float* pred, const void* target, int target_u8, int batch, int channels, int hw,
                                    const double* sums, const float* grad_out, float* grad, int device, void* stream) {
    dad3d_status st = iou_check("dad3d_heatmap_iou_grad", pred, target, target_u8, batch, channels, hw);
    if (st) return st;
    if (batch == 0 || channels == 0 || hw == 0) return DAD3D_OK;
    DAD3D_REQUIRE(sums && grad_out && grad, "dad3d_heatmap_iou_grad: null argument");
    DAD3D_SELECT_DEVICE(device);
    IouArgs a{pred, target, const_cast<double*>(sums), nullptr, nullptr, nullptr, grad_out, grad, (size_t)batch * channels, hw,
              target_u8 != 0};
    return launch_heatmap_iou_grad(a, iou_vec(pred, target, target_u8, hw) && aligned(grad, 16), static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_visibility_point_loss(const float* pred, const float* pred_presence, const float* target,
                                         const float* target_presence, int batch, int n_points, int criterion, float* loss,
                                         float* grad_pred, int device, void* stream) {
    DAD3D_REQUIRE(batch >= 0 && n_points >= 0, "dad3d_visibility_point_loss: negative size");
    DAD3D_REQUIRE(criterion >= DAD3D_LOSS_L1 && criterion <= DAD3D_LOSS_SMOOTH_L1, "dad3d_visibility_point_loss: unknown criterion %d",
                  criterion);
    DAD3D_REQUIRE(batch > 0 && n_points > 0, "dad3d_visibility_point_loss: no points (the reference's mean over none is NaN)");
    DAD3D_REQUIRE(pred && pred_presence && target && target_presence && loss, "dad3d_visibility_point_loss: null argument");
    DAD3D_SELECT_DEVICE(device);
    VisibilityLossArgs a{pred, pred_presence, target, target_presence, loss, grad_pred, batch, n_points, criterion};
    return launch_visibility_loss(a, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_keypoint_errors(const float* pred, const float* target, int batch, int n_verts, int dims, const int32_t* index,
                                   int n_points, const float* presence, float pred_scale, float target_scale, int cube,
                                   const int32_t* bbox, const double* thresholds, int n_thresholds, int below, double* err,
                                   float* out, float* accum, int device, void* stream) {
    DAD3D_REQUIRE(batch > 0 && n_verts > 0 && n_points > 0, "dad3d_keypoint_errors: bad size (batch %d, n_verts %d, n_points %d)",
                  batch, n_verts, n_points);
    DAD3D_REQUIRE(batch <= 0x7fffffff && (dims == 2 || dims == 3), "dad3d_keypoint_errors: dims must be 2 or 3, not %d", dims);
    DAD3D_REQUIRE(index || n_points <= n_verts, "dad3d_keypoint_errors: %d points of %d vertices", n_points, n_verts);
    DAD3D_REQUIRE(n_thresholds >= 0 && n_thresholds <= kMaxThresholds, "dad3d_keypoint_errors: %d thresholds (at most %d)", n_thresholds,
                  kMaxThresholds);
    DAD3D_REQUIRE(!cube || dims == 3, "dad3d_keypoint_errors: normalize_to_cube needs 3-D points");
    DAD3D_REQUIRE(pred && target && err && (n_thresholds == 0 || thresholds), "dad3d_keypoint_errors: null argument");
    DAD3D_REQUIRE(!accum || out, "dad3d_keypoint_errors: accum needs out");
    DAD3D_SELECT_DEVICE(device);
    KeypointErrArgs a{};
    a.pred = pred, a.target = target, a.index = index, a.presence = presence, a.bbox = bbox, a.err = err, a.out = out,
    a.accum = accum;
    a.pred_scale = pred_scale, a.target_scale = target_scale;
    for (int k = 0; k < n_thresholds; ++k) a.thresholds[k] = thresholds[k];  // HOST array
    a.batch = batch, a.n_verts = n_verts, a.n_points = n_points, a.dims = dims, a.n_thresholds = n_thresholds;
    a.cube = cube != 0, a.below = below != 0;
    return launch_keypoint_errors(a, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_eval_nearest(const float* query, const float* points, const int32_t* counts, const float* similarity,
                                int batch, int n_query, int n_points, int k, int flags, float* min_dist2, int32_t* knn_index,
                                float* knn_dist2, int device, void* stream) {
    DAD3D_REQUIRE(batch > 0 && n_query > 0 && n_points > 0, "dad3d_eval_nearest: sizes must be positive (B %d, Q %d, N %d)", batch,
                  n_query, n_points);
    DAD3D_REQUIRE(k >= 1 && k <= kEvalMaxK, "dad3d_eval_nearest: k = %d outside 1..%d", k, kEvalMaxK);
    DAD3D_REQUIRE((flags & ~DAD3D_EVAL_SELF_EXCLUDE) == 0, "dad3d_eval_nearest: unknown flags 0x%x", flags);
    DAD3D_REQUIRE(query && points && min_dist2, "dad3d_eval_nearest: null argument");
    DAD3D_REQUIRE(batch <= 65535, "dad3d_eval_nearest: batch beyond the launch grid");
    DAD3D_REQUIRE(!(flags & DAD3D_EVAL_SELF_EXCLUDE) || n_query == n_points,
                  "dad3d_eval_nearest: DAD3D_EVAL_SELF_EXCLUDE needs the same set as query and points (Q %d, N %d)", n_query, n_points);
    DAD3D_SELECT_DEVICE(device);
    EvalNearestArgs a{query, points, counts, similarity, min_dist2, knn_index, knn_dist2, batch, n_query, n_points, k,
                      (flags & DAD3D_EVAL_SELF_EXCLUDE) ? 1 : 0};
    return launch_eval_nearest(a, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_eval_z5_ranks(const float* gt_head, const float* pred_head, int batch, int n_head, const int32_t* anchors,
                                 int n_anchors, int32_t* counts, int32_t* order, int device, void* stream) {
    DAD3D_REQUIRE(batch > 0 && n_head > 0, "dad3d_eval_z5_ranks: sizes must be positive (B %d, K %d)", batch, n_head);
    DAD3D_REQUIRE(n_head <= kEvalMaxHead, "dad3d_eval_z5_ranks: K = %d head vertices exceed the %d the LDS sort holds", n_head,
                  kEvalMaxHead);
    DAD3D_REQUIRE(n_anchors >= 1 && n_anchors <= kEvalMaxAnchors, "dad3d_eval_z5_ranks: %d anchors outside 1..%d", n_anchors,
                  kEvalMaxAnchors);
    DAD3D_REQUIRE(gt_head && pred_head && anchors && counts, "dad3d_eval_z5_ranks: null argument");
    DAD3D_REQUIRE(batch <= 65535, "dad3d_eval_z5_ranks: batch beyond the launch grid");
    EvalZ5Args a{gt_head, pred_head, counts, order, {}, batch, n_head, 1, n_anchors};
    for (int i = 0; i < n_anchors; ++i) {
        DAD3D_REQUIRE(anchors[i] >= 0 && anchors[i] < n_head, "dad3d_eval_z5_ranks: anchor %d = %d outside 0..%d", i, anchors[i],
                      n_head - 1);
        a.anchors[i] = anchors[i];
    }
    while (a.sort_len < n_head) a.sort_len <<= 1;
    DAD3D_SELECT_DEVICE(device);
    return launch_eval_z5(a, static_cast<hipStream_t>(stream));
}

// ---- head pose and similarity alignment (head_pose.hip) -----------------------------------------------------------------
static dad3d_status head_pose_check(const char* who, const float* params, int n, int64_t row_stride, int rot_offset, const int64_t* frames,
                                    int n_frames, const int32_t* image_index, int h, int w, const double* rpy, const float* points) {
    DAD3D_REQUIRE(n >= 0 && row_stride >= 0 && rot_offset >= 0, "%s: negative size (n %d, row_stride %lld, rot_offset %d)", who, n,
                  (long long)row_stride, rot_offset);
    if (n == 0) return DAD3D_OK;
    DAD3D_REQUIRE(params, "%s: null params", who);
    DAD3D_REQUIRE(aligned(params, 4) && aligned(rpy, 8) && aligned(points, 4), "%s: params / rpy / points are not aligned to their elements", who);
    DAD3D_REQUIRE((frames != nullptr) == (image_index != nullptr), "%s: the frame table and image_index come together", who);
    DAD3D_REQUIRE(!frames || n_frames >= 0, "%s: n_frames %d is negative", who, n_frames);
    DAD3D_REQUIRE(!points || frames || (h >= 1 && w >= 1), "%s: points need a frame table or one frame size, got %d x %d", who, h, w);
    return DAD3D_OK;
}

dad3d_status dad3d_head_pose(const float* params, int n, int64_t row_stride, int rot_offset, const int64_t* frames, int n_frames,
                             const int32_t* image_index, int h, int w, float* rotation, double* rpy, float* points, int32_t* flags,
                             int device, void* stream) {
    const dad3d_status st = head_pose_check("dad3d_head_pose", params, n, row_stride, rot_offset, frames, n_frames, image_index, h, w, rpy, points);
    if (st != DAD3D_OK || n == 0) return st;
    DAD3D_SELECT_DEVICE(device);
    HeadPoseArgs a{params, (long long)row_stride, rot_offset, n, reinterpret_cast<const long long*>(frames), image_index, n_frames, h, w,
                   rotation, rpy, points, flags};
    return launch_head_pose(a, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_head_pose_host(const float* params, int n, int64_t row_stride, int rot_offset, const int64_t* frames, int n_frames,
                                  const int32_t* image_index, int h, int w, float* rotation, double* rpy, float* points, int32_t* flags) {
    const dad3d_status st = head_pose_check("dad3d_head_pose_host", params, n, row_stride, rot_offset, frames, n_frames, image_index, h, w, rpy, points);
    if (st != DAD3D_OK || n == 0) return st;
    HeadPoseArgs a{params, (long long)row_stride, rot_offset, n, reinterpret_cast<const long long*>(frames), image_index, n_frames, h, w,
                   rotation, rpy, points, flags};
    head_pose_host(a);
    return DAD3D_OK;
}

static dad3d_status procrustes_check(const char* who, const double* x, const double* y, int batch, int n_points, const double* b, const double* t,
                                     const double* c, const int32_t* flags) {
    DAD3D_REQUIRE(batch >= 0 && n_points >= 1, "%s: bad size (batch %d, n_points %d)", who, batch, n_points);
    DAD3D_REQUIRE((long long)batch * n_points * 3 <= 0x7fffffffLL, "%s: %d x %d points are beyond 2^31 values", who, batch, n_points);
    if (batch == 0) return DAD3D_OK;
    DAD3D_REQUIRE(x && y && b && t && c && flags, "%s: null argument", who);
    DAD3D_REQUIRE(aligned(x, 8) && aligned(y, 8) && aligned(b, 8) && aligned(t, 8) && aligned(c, 8), "%s: float64 arrays must be 8-byte aligned", who);
    return DAD3D_OK;
}

dad3d_status dad3d_procrustes(const double* x, const double* y, int batch, int n_points, double* b, double* t, double* c, int32_t* flags,
                              int device, void* stream) {
    const dad3d_status st = procrustes_check("dad3d_procrustes", x, y, batch, n_points, b, t, c, flags);
    if (st != DAD3D_OK || batch == 0) return st;
    DAD3D_SELECT_DEVICE(device);
    ProcrustesArgs a{x, y, batch, n_points, b, t, c, flags};
    return launch_procrustes(a, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_procrustes_host(const double* x, const double* y, int batch, int n_points, double* b, double* t, double* c, int32_t* flags) {
    const dad3d_status st = procrustes_check("dad3d_procrustes_host", x, y, batch, n_points, b, t, c, flags);
    if (st != DAD3D_OK || batch == 0) return st;
    ProcrustesArgs a{x, y, batch, n_points, b, t, c, flags};
    procrustes_host(a);
    return DAD3D_OK;
}

}  // extern "C"
