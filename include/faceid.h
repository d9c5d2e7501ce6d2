/*
 * faceid.h -- C ABI of libfaceid.so: the MI355X (gfx950) implementation of the
 * detect -> align -> embed -> match hot path of Kumar2421/scrfd_arcface_facerecognition.
 *
 * The reference has no native boundary of its own: its hot path is Python that calls into
 * onnxruntime / OpenCV / scikit-image / numpy.  Each entry point below replaces one of those
 * third-party calls (cited as reference file:line) and is what the ctypes binding in
 * scrfd_arcface_facerecognition_amd/_lib.py loads (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - every function returns 0 (FID_OK) or a negative FID_E_* code; no exception crosses the ABI;
 *     fid_last_error() gives the message for the calling thread's last failure.
 *   - pointers named *_dev are DEVICE pointers (from fid_malloc, or any HIP allocation such as a
 *     torch tensor's data_ptr()); everything else is host memory owned by the caller.
 *   - all work is enqueued on the context's HIP stream and is asynchronous unless the function
 *     copies to host memory (fid_memcpy_d2h, fid_*_read) or is fid_sync().
 *   - a context is not re-entrant: calls on the same fid_ctx are serialised by an internal mutex;
 *     different contexts are independent (one process per GPU in the multi-GPU runs).
 *   - images are uint8, H x W x 3, BGR, dense (the layout cv2.imread / VideoCapture.read return,
 *     reference main.py:95,176).
 */
#ifndef FACEID_H
#define FACEID_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FID_ABI_VERSION 2   /* 2: fid_face_gates takes the pose angles as float64 (round 4) */

#define FID_OK 0
#define FID_E_INVALID (-1)   /* bad argument / shape / table */
#define FID_E_HIP (-2)       /* HIP runtime error (message has the hipError string) */
#define FID_E_CAPACITY (-3)  /* caller-provided capacity too small */
#define FID_E_NOMEM (-4)
#define FID_E_STATE (-5)     /* object used in the wrong state */

typedef struct fid_ctx fid_ctx;         /* device + stream + scratch */
typedef struct fid_net fid_net;         /* a compiled conv net (layer table + packed weights) */
typedef struct fid_gallery fid_gallery; /* L2-normalised fp16 gallery resident in HBM */
typedef struct fid_comm fid_comm;       /* one rank of an RCCL communicator (one process per GPU) */

/* ---- library / context -------------------------------------------------------------------- */
int fid_abi_version(void);
const char *fid_last_error(void);
int fid_device_count(int *count);
/* stream: an existing hipStream_t to enqueue on (e.g. torch's current stream), or NULL to let
 * the context create its own non-blocking stream. */
int fid_ctx_create(int device, void *stream, fid_ctx **out);
int fid_ctx_destroy(fid_ctx *ctx);
int fid_sync(fid_ctx *ctx);
int fid_device_name(fid_ctx *ctx, char *buf, int buflen);

/* ---- device memory (so a host without torch can drive the library) -------------------------- */
int fid_malloc(fid_ctx *ctx, size_t bytes, void **dptr);
int fid_free(fid_ctx *ctx, void *dptr);
int fid_memcpy_h2d(fid_ctx *ctx, void *dst_dev, const void *src, size_t bytes);
int fid_memcpy_d2h(fid_ctx *ctx, void *dst, const void *src_dev, size_t bytes); /* synchronises */
int fid_memset(fid_ctx *ctx, void *dst_dev, int value, size_t bytes);

/* ---- pinned host staging + an upload stream: double-buffered H2D for the video front-end (the step before the
 * path: reference main.py:174-184 reads and uploads one frame at a time).  fid_upload_async copies on a separate
 * HIP stream, ordered after the compute work enqueued so far (the destination may still be in use);
 * fid_upload_wait makes the compute stream wait for it -- no host synchronisation in either. */
int fid_pinned_alloc(fid_ctx *ctx, size_t bytes, void **hptr);
int fid_pinned_free(fid_ctx *ctx, void *hptr);
int fid_upload_async(fid_ctx *ctx, void *dst_dev, const void *src_pinned, size_t bytes);
int fid_upload_wait(fid_ctx *ctx);
/* Per-buffer ordering for double buffering (slot = one device staging buffer, 0 <= slot < FID_UPLOAD_SLOTS):
 * fid_upload_release(slot) marks the compute work enqueued so far as the last reader of that buffer;
 * fid_upload_async_slot copies into it after ONLY that release (so the upload of batch i+1 overlaps the compute of
 * batch i, which reads the other buffer); fid_upload_wait_slot makes the compute stream wait for that upload. */
#define FID_UPLOAD_SLOTS 4
int fid_upload_release(fid_ctx *ctx, int slot);
int fid_upload_async_slot(fid_ctx *ctx, int slot, void *dst_dev, const void *src_pinned, size_t bytes);
int fid_upload_wait_slot(fid_ctx *ctx, int slot);

/* ---- timing with HIP events on the context's stream (bench.py roofline leg) ----------------- */
#define FID_MAX_EVENTS 64
int fid_event_record(fid_ctx *ctx, int slot);
int fid_event_elapsed_ms(fid_ctx *ctx, int slot_start, int slot_stop, float *ms); /* synchronises */

/* ---- conv nets: replaces onnxruntime.InferenceSession(...).run ------------------------------
 * reference models/scrfd.py:59-62,83 and models/arcface.py:18-21,51.
 * The net is described by a layer table produced by scrfd_arcface_facerecognition_amd/lower.py
 * (format documented in csrc/net.h): `ops` is n_ops x FID_OP_WORDS int32, `tensors` is
 * n_tensors x FID_TENSOR_WORDS int32, `blob` holds packed fp16 weights + fp32 epilogue tables.
 * Input of fid_net_run: uint8 BGR images [batch, H, W, 3]; the blob conversion
 * (cv2.dnn.blobFromImage(s), scrfd.py:76-82 / arcface.py:44-50) is fused into the first conv.
 * A net belongs to the context it was created with: its activation slots, lazily built weight repackings and kernel plans
 * are per net and unsynchronised, so run one net from ONE context (several host threads may share that context: its mutex
 * serialises them); a second stream needs its own fid_net (bench.py: one per lane). */
#define FID_OP_WORDS 32
#define FID_TENSOR_WORDS 8
int fid_net_create(fid_ctx *ctx, const int32_t *ops, int n_ops, const int32_t *tensors,
                   int n_tensors, const void *blob, size_t blob_bytes, int in_h, int in_w,
                   int max_batch, fid_net **out);
int fid_net_destroy(fid_ctx *ctx, fid_net *net);
int fid_net_run(fid_ctx *ctx, fid_net *net, const uint8_t *images_dev, int batch);
/* Execute depth-first over sub-batches of this many images (0 = the whole batch layer by layer), so
 * that a layer's input is still in L2 / Infinity Cache when the next layer reads it. */
int fid_net_set_sub_batch(fid_net *net, int sub_batch);
/* device address + geometry of a tensor of the last run: dims = {H, W, C_logical, C_stored},
 * dtype 0 = fp16, 1 = fp32; layout [batch, H, W, C_stored]. */
int fid_net_tensor(fid_net *net, int tensor_id, void **dptr, int dims[4], int *dtype);
/* per-op device time of the last fid_net_run_profiled (ms per op, n_ops floats) */
int fid_net_run_profiled(fid_ctx *ctx, fid_net *net, const uint8_t *images_dev, int batch,
                         float *op_ms);
/* Kernel plans (per conv op and batch size the executor times its candidate kernels at first use and keeps the fastest).
 * Text lines keyed by ISA name + CU count + layer-table hash (incl. the library's candidate-set revision); every line is checked
 * against this library's candidates before its first use; a loaded plan replaces the timing, so two boxes run the same
 * kernels / fp32 summation orders and return bit-identical outputs.  Environment FID_PLAN=<file>: load at
 * fid_net_create, append every new pick; FID_PLAN_RO=<file>: load only.  (No reference analogue: onnxruntime picks its kernels internally.) */
int fid_net_plan_save(fid_net *net, const char *path);
int fid_net_plan_load(fid_net *net, const char *path, int *n_loaded);
/* algorithmic cost of one image through the net: multiply-accumulates (true channel counts) */
int fid_net_macs(fid_net *net, double *macs_per_image);

/* ---- letterbox: replaces cv2.resize + zero paste, reference models/scrfd.py:123-138 ---------
 * frames [B,H,W,3] -> out [B,in_h,in_w,3]; det_scale (new_h / H, as a double) is returned. */
int fid_letterbox(fid_ctx *ctx, const uint8_t *frames_dev, int B, int H, int W,
                  uint8_t *out_dev, int in_h, int in_w, double *det_scale);

/* ---- mixed-size batches: the *_ragged forms of fid_letterbox, fid_scrfd_postprocess, fid_align_crops and fid_align_crops_packed.
 * The reference does all of these per image (build_targets, main.py:78-105, calls detect() and the recogniser once per photo); here one
 * call takes B images of B different sizes.  A mixed batch is ONE device allocation plus two HOST arrays:
 *   hw      int32 [B,2]  H_b, W_b
 *   offsets int64 [B]    image b is dense uint8 [H_b, W_b, 3] BGR, its first byte at frames_dev + offsets[b]
 * frames_bytes is the size of the allocation: no byte at or beyond it is ever read.  Images may overlap or repeat; the offsets need
 * no alignment.  Validation is all-or-nothing: H, W <= 0, offsets[b] < 0, offsets[b] + H*W*3 > frames_bytes or a letterbox with
 * new_h == 0 or new_w == 0 return FID_E_INVALID with the image index in fid_last_error(), and nothing is enqueued.  The per-image
 * geometry is computed on the host in double, as fid_letterbox / fid_scrfd_postprocess compute it, and travels to a device table
 * the context owns, ordered on the context's stream: hw and offsets may be freed or overwritten as soon as a call returns, calls
 * enqueued back to back each read their own table, and no call synchronises with the host.  Limits on B, slots and rows as in the
 * uniform calls; one kernel launch per stage for the whole batch.
 *
 * fid_letterbox_ragged: reference models/scrfd.py:123-138 per image; out [B,in_h,in_w,3]; det_scale: host [B] (new_h_b / H_b), may be NULL. */
int fid_letterbox_ragged(fid_ctx *ctx, const uint8_t *frames_dev, size_t frames_bytes, const int32_t *hw, const int64_t *offsets,
                         int B, uint8_t *out_dev, int in_h, int in_w, double *det_scale);

/* ---- tiled detection: frames larger than the detector input, seen at the resolution they were filmed in.  (No reference analogue:
 * models/scrfd.py:123-138 letterboxes the whole frame, so a 1080p frame reaches a 640x640 detector at one third of its scale.)
 * A tile table is a HOST int32 [T,6] array, one row per tile: frame, x0, y0, w, h, kind.
 *   kind 0  native: the rectangle (x0, y0, w, h) of frame `frame` is copied 1:1 to the top-left of the detector input, the rest of the
 *           input is zero; w <= in_w, h <= in_h; its det_scale is exactly 1.0f.
 *   kind 1  letterboxed: the rectangle is resized into the input with the geometry and pixel arithmetic fid_letterbox uses for an h x w
 *           image; det_scale = (float)(new_h / (double)h).  A kind 1 row that covers a whole frame is byte for byte fid_letterbox of it.
 * Rows of one frame are contiguous and frames appear in ascending order; the position of a row within its frame is its tile rank.
 * Validation is all-or-nothing: a frame outside [0, B), a rectangle not inside the frame, w or h <= 0, a kind 0 tile larger than the input,
 * a degenerate letterbox, rows not grouped by ascending frame or an unknown kind return FID_E_INVALID with the row index in
 * fid_last_error(), and nothing is enqueued.  The table travels to a device table the context owns, ordered on the context's stream: it
 * may be freed or overwritten as soon as a call returns, and no call synchronises with the host.  T <= 65535.
 *
 * fid_tile_cut: frames [B,H,W,3] -> out [T,in_h,in_w,3], one launch for all tiles; no byte outside frames is read. */
int fid_tile_cut(fid_ctx *ctx, const uint8_t *frames_dev, int B, int H, int W, const int32_t *tiles, int T,
                 uint8_t *out_dev, int in_h, int in_w);

/* ---- NV12 video frames: what a video decoder hands out, taken as it is.  (No reference analogue: the reference's frames come from
 * cv2.VideoCapture.read(), main.py:174-184, which converts the decoder's NV12 to BGR on the host before the reference sees a pixel.)
 * An NV12 frame is a full-resolution Y plane and a half-resolution plane of interleaved U, V pairs, 1.5 bytes per pixel, rows `pitch`
 * bytes apart in both planes.  B frames are ONE allocation described by fid_nv12_desc; H and W are even.
 *
 * The conversion is integer only and is OpenCV's COLOR_YUV2BGR_NV12, so the bytes are those a host-side cvtColor gave before.  Chroma is
 * replicated, not interpolated: pixel (y, x) uses Y[y][x], U = UV[y>>1][(x>>1)*2], V = UV[y>>1][(x>>1)*2 + 1].  With a standard's table
 * {CY, CUB, CUG, CVG, CVR, Y0}:
 *   yy = max(0, Y - Y0) * CY;   u = U - 128;   v = V - 128
 *   B = sat8((yy + CUB*u + (1 << 19)) >> 20)
 *   G = sat8((yy + CUG*u + CVG*v + (1 << 19)) >> 20)
 *   R = sat8((yy + CVR*v + (1 << 19)) >> 20)             >> is the arithmetic shift, sat8 clamps to 0 .. 255.
 * Each integer is floor(c * 2^20 + 0.5) of its coefficient: BT.601 limited range 1.164, 2.018, -0.391, -0.813, 1.596 (OpenCV's own); BT.709
 * limited range 1.164, 2.112, -0.213, -0.533, 1.793; BT.601 full range (MJPEG cameras) 1.0, 1.772, -0.344136, -0.714136, 1.402, Y0 = 0. */
#define FID_YUV_BT601_LIMITED 0
#define FID_YUV_BT709_LIMITED 1
#define FID_YUV_BT601_FULL 2
#define FID_YUV_BT601_LIMITED_TABLE {1220542, 2116026, -409993, -852492, 1673527, 16}
#define FID_YUV_BT709_LIMITED_TABLE {1220542, 2214593, -223347, -558891, 1880097, 16}
#define FID_YUV_BT601_FULL_TABLE {1048576, 1858077, -360853, -748826, 1470104, 0}
typedef struct fid_nv12_desc {
    int32_t pitch;                 /* bytes from one row to the next, in both planes; >= W */
    int64_t uv_offset;             /* from a frame's first Y byte to its first UV byte; >= pitch * H (decoders align the plane height) */
    int64_t frame_stride;          /* bytes from one frame to the next; >= uv_offset + pitch * H / 2 */
    int32_t standard;              /* FID_YUV_* */
} fid_nv12_desc;
/* Of frame b only the bytes [b * frame_stride, b * frame_stride + uv_offset + pitch * H / 2) can be read, and of each row only its first W
 * bytes: padding behind the last UV row, between W and pitch, between the planes and between the frames is never read.  The planes are read
 * bytewise: pitch, uv_offset, frame_stride and the allocation need no alignment.  Validation is all-or-nothing, like the ragged calls: a NULL
 * layout, an odd H or W, pitch < W, planes or frames that overlap (the two >= above) or an unknown standard return FID_E_INVALID with a message
 * in fid_last_error(), and nothing is enqueued.  desc is HOST memory, read before the call returns.
 *
 * fid_nv12_to_bgr: nv12 -> dense uint8 [B,H,W,3] BGR on the device, one launch; B, H <= 65535.  fid_nv12_to_bgr_host: the same definition in
 * plain loops on HOST arrays, no device involved.
 * fid_letterbox_nv12, fid_tile_cut_nv12, fid_align_crops_nv12, fid_align_crops_packed_nv12: the arguments of their BGR namesakes with
 * (nv12_dev, desc) in place of frames_dev.  EACH WRITES EXACTLY THE BYTES ITS NAMESAKE WRITES WHEN GIVEN fid_nv12_to_bgr OF THE SAME FRAMES
 * (det_scale and the rows of M_dev included), with no BGR frame in device memory: every tap is converted first and interpolated second, with
 * the namesake's own fixed-point arithmetic -- the identity copy, the exact-2x sum of four converted pixels, the zero fill outside
 * new_w x new_h and the warp's zero for a tap outside the frame included.  The mixed-size (_ragged) forms have no NV12 twin. */
int fid_nv12_to_bgr(fid_ctx *ctx, const uint8_t *nv12_dev, const fid_nv12_desc *desc, int B, int H, int W, uint8_t *bgr_out_dev);
int fid_nv12_to_bgr_host(const uint8_t *nv12, const fid_nv12_desc *desc, int B, int H, int W, uint8_t *bgr_out);
int fid_letterbox_nv12(fid_ctx *ctx, const uint8_t *nv12_dev, const fid_nv12_desc *desc, int B, int H, int W,
                       uint8_t *out_dev, int in_h, int in_w, double *det_scale);
int fid_tile_cut_nv12(fid_ctx *ctx, const uint8_t *nv12_dev, const fid_nv12_desc *desc, int B, int H, int W, const int32_t *tiles, int T,
                      uint8_t *out_dev, int in_h, int in_w);
int fid_align_crops_nv12(fid_ctx *ctx, const uint8_t *nv12_dev, const fid_nv12_desc *desc, int B, int H, int W,
                         const float *kps_dev, const int32_t *counts_dev, int cap, int faces_per_frame,
                         uint8_t *crops_dev, double *M_dev);
int fid_align_crops_packed_nv12(fid_ctx *ctx, const uint8_t *nv12_dev, const fid_nv12_desc *desc, int B, int H, int W, const float *kps_dev,
                                int cap, const int32_t *src_dev, int n_rows, uint8_t *crops_dev, double *M_dev);

/* ---- BGR -> NV12: the way out, for an encoder that wants the decoder's own format (the reference hands BGR frames to cv2.VideoWriter,
 * main.py:174-184, which converts on the host).  The forward definition is integer only, like the inverse above.  With kr, kb the standard's
 * luma weights (BT.601: 0.299, 0.114; BT.709: 0.2126, 0.0722), kg = 1 - kr - kb, and (ys, cs) = (219/255, 224/255) for the limited ranges,
 * (1, 1) for the full range, a standard's table {YB, YG, YR, UB, UG, UR, VB, VG, VR, Y0} holds floor(c * 2^20 + 0.5) of
 *   Y row   ys * (kb, kg, kr)
 *   U row   cs * 0.5 * (1, -kg / (1 - kb), -kr / (1 - kb))
 *   V row   cs * 0.5 * (-kb / (1 - kr), -kg / (1 - kr), 1)          each on (B, G, R); the U row and the V row sum to 0.
 * Luma of pixel (B, G, R):      Y = sat8((YB*B + YG*G + YR*R + (Y0 << 20) + (1 << 19)) >> 20)
 * Chroma of a 2 x 2 group whose four pixels sum to (SB, SG, SR), each 0 .. 1020 -- the box-filtered sample, the one the inverse replicates:
 *                               U = sat8((UB*SB + UG*SG + UR*SR + (128 << 22) + (1 << 21)) >> 22),  V likewise with the V row.
 * Every sum stays below 1.08e9 in magnitude (int32); every grey maps to U = V = 128 exactly.  One solid colour c: Y(c), and the (U, V) of the
 * flat group S = 4 * c.  fid_nv12_to_bgr of fid_bgr_to_nv12 of a frame of flat 2 x 2 blocks is within 2 levels of it per channel. */
#define FID_YUV_BT601_LIMITED_FWD_TABLE {102662, 528618, 269262, 460551, -305128, -155423, -74897, -385654, 460551, 16}
#define FID_YUV_BT709_LIMITED_FWD_TABLE {65019, 644067, 191455, 460551, -355018, -105533, -42230, -418321, 460551, 16}
#define FID_YUV_BT601_FULL_FWD_TABLE {119538, 615514, 313524, 524288, -347356, -176932, -85262, -439026, 524288, 0}
/* fid_bgr_to_nv12: dense uint8 [B,H,W,3] BGR on the device -> B frames in the layout `desc` (checked like every NV12 layout above: H and W
 * even ...), one launch; B <= 65535.  It writes the first W bytes of every Y row and of every UV row of the layout and NOTHING else: padding
 * between W and pitch, between the planes, behind the last UV row and between the frames keeps its bytes.  The two buffers must not overlap.
 * FID_E_INVALID, nothing enqueued: a NULL pointer, a bad layout, overlapping buffers.  fid_bgr_to_nv12_host: the same in plain loops on HOST
 * arrays. */
int fid_bgr_to_nv12(fid_ctx *ctx, const uint8_t *bgr_dev, int B, int H, int W, uint8_t *nv12_out_dev, const fid_nv12_desc *desc);
int fid_bgr_to_nv12_host(const uint8_t *bgr, int B, int H, int W, uint8_t *nv12_out, const fid_nv12_desc *desc);

/* ---- SCRFD post-process: replaces the numpy code of reference models/scrfd.py:89-178,180-207
 * and utils/helpers.py:62-107 (threshold, distance2bbox/kps decode, sort, greedy NMS, max_num).
 * The 9 head tensors (scores, bbox, kps for strides 8/16/32) are given as strided views so both
 * the ONNX layout ([H*W*A,1|4|10]) and the executor's fused NHWC head tensor can be read:
 *   element(frame b, anchor i, component c) =
 *       ptr[k][ b*batch_stride[k] + (i / A)*pix_stride[k] + (i % A)*anc_stride[k] + c ]
 * Outputs (device): det [B,cap,5] (x1,y1,x2,y2,score), kps [B,cap,10], counts [B].
 * All frames of one call share the original image size (img_h,img_w) -- they are one dense array.
 * metric: 0 = "max" (area), 1 = area - 2*centre_dist^2 (scrfd.py:169-172).
 * Returns FID_E_CAPACITY (after the fact, via fid_scrfd_check) if a frame had more survivors
 * than `cap` or more candidates than cand_cap. */
int fid_scrfd_postprocess(fid_ctx *ctx, const float *const head_dev[9], const int32_t pix_stride[9],
                          const int32_t anc_stride[9], const int64_t batch_stride[9], int B,
                          int in_h, int in_w, int num_anchors, int img_h, int img_w, float conf_thres,
                          float iou_thres, int max_num, int metric, float *det_dev, float *kps_dev,
                          int32_t *counts_dev, int cap);
/* The same for a mixed-size batch: frame b is the letterbox of an H_b x W_b image (hw: host int32 [B,2]).  Reference
 * models/scrfd.py:145-148 (the division by that image's det_scale) and :159-177 (max_num around that image's centre), which the reference
 * runs per image; sort, NMS and the capacity report through fid_scrfd_check are those of fid_scrfd_postprocess. */
int fid_scrfd_postprocess_ragged(fid_ctx *ctx, const float *const head_dev[9], const int32_t pix_stride[9],
                                 const int32_t anc_stride[9], const int64_t batch_stride[9], int B, int in_h, int in_w,
                                 int num_anchors, const int32_t *hw, float conf_thres, float iou_thres, int max_num, int metric,
                                 float *det_dev, float *kps_dev, int32_t *counts_dev, int cap);
/* The same for tiled detection: the head tensors have batch dimension T (the detector's run over fid_tile_cut's output), the outputs
 * batch dimension B, in fid_scrfd_postprocess's layout; tiles is the table fid_tile_cut took, the frames are img_h x img_w.  Tile t decodes
 * as a frame of fid_scrfd_postprocess does with its own det_scale; every coordinate v then becomes (v / det_scale) + (float)x0 (y0 for y
 * values), two single rounded fp32 operations, and the candidate joins the list of the tile's frame.  Inside a frame equal scores fall in
 * (tile rank, anchor) order; tiles per frame x anchors must stay below 2^31.
 * Edge rule (m = edge_margin; m < 0 switches it off), on the frame-coordinate box in fp32: a candidate is dropped before it takes a slot if
 *   x0 > 0 && x1 < x0 + m,   y0 > 0 && y1 < y0 + m,   x0 + w < img_w && x2 > x0 + w - m   or   y0 + h < img_h && y2 > y0 + h - m
 * -- the half faces a tile sees at a cut; a side that lies on the frame's boundary never rejects.
 * Sort, NMS (one per frame, over the candidates of all its tiles), max_num around the FRAME's centre and the capacity report through
 * fid_scrfd_check are those of fid_scrfd_postprocess: cand_cap bounds the candidates of a frame's tiles together.  A table of one kind 1 row
 * per frame that covers it gives fid_scrfd_postprocess's det, kps and counts. */
int fid_scrfd_postprocess_tiled(fid_ctx *ctx, const float *const head_dev[9], const int32_t pix_stride[9],
                                const int32_t anc_stride[9], const int64_t batch_stride[9], const int32_t *tiles, int T,
                                int in_h, int in_w, int num_anchors, int B, int img_h, int img_w, float conf_thres, float iou_thres,
                                int edge_margin, int max_num, int metric, float *det_dev, float *kps_dev, int32_t *counts_dev, int cap);
/* candidates per frame the sort/NMS workspace is sized for (default 4096; max 16800 = all anchors
 * of a 640x640 input) */
int fid_scrfd_set_candidate_capacity(fid_ctx *ctx, int cand_cap);
/* synchronises and reports overflow of the last fid_scrfd_postprocess: max candidates seen */
int fid_scrfd_check(fid_ctx *ctx, int *max_candidates);
/* SCRFD.forward's decode loop alone (reference models/scrfd.py:89-119): the candidates with
 * score >= conf_thres in anchor order (levels 8,16,32 concatenated), NOT divided by det_scale.
 * rec_dev: [B, cand_cap, 16] floats = x1 y1 x2 y2 score kps[10] flat-anchor-index(int bits). */
int fid_scrfd_decode(fid_ctx *ctx, const float *const head_dev[9], const int32_t pix_stride[9],
                     const int32_t anc_stride[9], const int64_t batch_stride[9], int B, int in_h,
                     int in_w, int num_anchors, float conf_thres, float *rec_dev, int32_t *counts_dev);
/* distance2bbox / distance2kps on plain device arrays (reference utils/helpers.py:62-107):
 * points [n,2], distance [n,4] / [n,ncol] -> out [n,4] / [n,ncol] */
int fid_distance2bbox(fid_ctx *ctx, const float *points_dev, const float *dist_dev, int n, float *out_dev);
int fid_distance2kps(fid_ctx *ctx, const float *points_dev, const float *dist_dev, int n, int ncol,
                     float *out_dev);
/* SCRFD.nms(dets, iou_thres) itself (reference models/scrfd.py:180-207): dets [K,5] device,
 * keep_dev receives indices into dets in keep order, count_dev[0] their number. */
int fid_nms(fid_ctx *ctx, const float *dets_dev, int K, float iou_thres, int32_t *keep_dev,
            int32_t *count_dev);

/* ---- alignment: replaces skimage SimilarityTransform.estimate + cv2.warpAffine +
 * cv2.dnn.blobFromImages' layout step; reference utils/helpers.py:18-59, arcface.py:54-57.
 * For frame b and face slot f < faces_per_frame: uses kps[b, f, :] if f < counts[b], else the
 * crop is zero-filled.  crops: uint8 [B*faces_per_frame, 112,112,3] BGR.  M_dev (optional, may
 * be NULL): the 2x3 double matrices estimate_norm would return, [B*faces_per_frame, 6].
 * A used slot whose landmarks admit no transform -- a NaN or infinite coordinate, or zero variance (five identical points) -- gets a
 * zero crop and an M row of six NaNs (an unused slot: zero crop, zero M); the other slots of the call are not affected.  The same holds
 * for the rows of the _ragged and _packed forms. */
int fid_align_crops(fid_ctx *ctx, const uint8_t *frames_dev, int B, int H, int W,
                    const float *kps_dev, const int32_t *counts_dev, int cap, int faces_per_frame,
                    uint8_t *crops_dev, double *M_dev);

/* The same for a mixed-size batch (reference utils/helpers.py:18-59, called per image): frame b is image b of the allocation; every
 * slot gets exactly the crop and M row fid_align_crops writes when called for that image alone. */
int fid_align_crops_ragged(fid_ctx *ctx, const uint8_t *frames_dev, size_t frames_bytes, const int32_t *hw, const int64_t *offsets, int B,
                           const float *kps_dev, const int32_t *counts_dev, int cap, int faces_per_frame, uint8_t *crops_dev, double *M_dev);

/* ---- packed face lists: every detected face of a batch as ONE dense row table, no per-frame padding.  The reference embeds every
 * face detect() returns (main.py:130-134: `detect(frame, params.max_num)` then `recognizer(frame, kps)` per face) and its default
 * max_num = 0 returns every NMS survivor (models/scrfd.py:159-177 selects only when max_num > 0); a B x faces_per_frame slot grid
 * pays for its most crowded frame in every frame.
 * fid_face_pack: k_b = min(max(counts[b], 0), cap) and, when max_per_frame > 0, also min(., max_per_frame).  offsets [B+1] = exclusive
 * prefix sum of k_b; offsets[B] = total faces, NOT clipped to row_cap (overflow is visible after the fact, as with fid_scrfd_check).
 * src [row_cap]: src[i] = b * cap + f -- the index of the i-th face, in (frame, rank) order, in det [B,cap,5] / kps [B,cap,10] of
 * fid_scrfd_postprocess -- for i < min(total, row_cap), -1 for the rows after them.  Faces beyond row_cap (the last ones in that
 * order) are dropped.  One launch; B * cap must fit an int32. */
int fid_face_pack(fid_ctx *ctx, const int32_t *counts_dev, int B, int cap, int max_per_frame,
                  int32_t *offsets_dev, int32_t *src_dev, int row_cap);
/* fid_align_crops driven by the row table (one recogniser input per face of main.py:130-134, all of models/scrfd.py:159-177's
 * survivors; the warp itself is utils/helpers.py:18-59): row i < n_rows with src[i] = b*cap+f >= 0
 * gets exactly the crop (and M row) fid_align_crops writes for face f of frame b; src[i] < 0 -> zero crop, zero M.
 * crops: uint8 [n_rows,112,112,3]; M_dev (optional, may be NULL): [n_rows, 6].  n_rows <= 65535. */
int fid_align_crops_packed(fid_ctx *ctx, const uint8_t *frames_dev, int B, int H, int W, const float *kps_dev, int cap,
                           const int32_t *src_dev, int n_rows, uint8_t *crops_dev, double *M_dev);

/* The row-table form for a mixed-size batch (the warp is reference utils/helpers.py:18-59, per image there): row i gets exactly the crop
 * and M row fid_align_crops_ragged writes for face f of frame b, src[i] = b*cap+f. */
int fid_align_crops_packed_ragged(fid_ctx *ctx, const uint8_t *frames_dev, size_t frames_bytes, const int32_t *hw, const int64_t *offsets,
                                  int B, const float *kps_dev, int cap, const int32_t *src_dev, int n_rows, uint8_t *crops_dev, double *M_dev);

/* ---- tracking faces across the frames of a video (reference main.py:174-184, two cameras in main2.py:91-99: the loop that detects, embeds and
 * matches EVERY face of EVERY frame).  A tracker decides on the device, in frame order, which detection continues which track and which faces
 * need an embedding now: a face that has been named keeps its name and is embedded again only every `refresh` frames.
 * A tracker is S streams (cameras) x T slots (1 <= T <= FID_TRACK_MAX_SLOTS), all state in device memory.  Per slot: id (int32, -1 = free), box
 * (the last matched detection), missed (frames since the last match), since (matches since the last embedding), ident_idx / ident_score (the
 * best gallery match over the track's life; -1 / 0 = unknown).  Per stream: next_id, lost (detections that found no slot).  A free slot has
 * id = -1 and every other word 0.
 * One step is  fid_track_step -> the consumers of the row table (fid_align_crops_packed, recogniser, fid_l2_normalize_f16_packed) -> fid_match
 * -> fid_track_identify;  a second step before the first one's identify, or an identify without a pending step, is FID_E_INVALID.
 *
 * fid_track_step.  det_dev [B,cap,5] / counts_dev [B]: as fid_scrfd_postprocess* writes them.  stream: HOST int32 [B], read before the call
 * returns (like hw of fid_scrfd_postprocess_ragged); stream[b] in [0, S) names the stream of frame b, frames of one stream stand in time order,
 * stream[b] < 0 skips the frame (no ageing, no rows, outputs -1).  Per stream, over its frames in batch order, k_b = min(max(counts[b], 0), cap):
 *   detections f = 0 .. k_b - 1 in order.  Candidates: the live tracks not yet matched in this frame (a track started in this frame counts as
 *     matched).  ovr(track.box, det) is the overlap of the post-process's NMS, operation for operation (areas with +1, intersection clamped at 0,
 *     correctly rounded divide).  A candidate hits when ovr > iou_thresh (strict: a NaN never hits); the best hit is the maximum ovr, lowest
 *     slot among equals.
 *       hit      track.box = det, missed = 0, since += 1; if since >= (known ? refresh : retry) the face is flagged EMBED and since = 0.  known =
 *                the track had ident_idx >= 0 after the last fid_track_identify (false for a track started during this call).
 *       no hit   the lowest free slot starts a track: id = next_id++, box = det, missed = since = 0, flags STARTED | EMBED.
 *       no slot  track id -1, slot -1, lost++, flagged EMBED: an untracked face is embedded every frame and reports its own match.
 *   end of frame: every live unmatched track gets missed += 1; missed > max_age frees the slot (usable from the stream's next frame on).
 * Outputs (device): track_dev int32 [B,cap,2] = {track id, slot | FID_TRACK_STARTED | FID_TRACK_EMBED} ({-1,-1}: an untracked face, an entry
 * f >= k_b, a skipped frame); the row table of the EMBED-flagged faces in (frame, rank) order in fid_face_pack's format: offsets_dev [B+1]
 * (offsets[B] = total, NOT clipped to row_cap), src_dev [row_cap] (b*cap+f, -1 behind the last row).  A flagged face beyond row_cap is not
 * embedded this time; its track keeps what it knows and asks again after the interval.
 *
 * fid_track_identify.  The step's stream, counts, track, offsets, src and sizes again, plus idx_dev / score_dev [n_rows] as fid_match wrote them
 * for the first n_rows rows of the table (n_rows = 0 with NULL idx / score: tracking without a gallery).  Per stream and frame, in order:
 * for the frame's rows i < min(offsets[b+1], n_rows, row_cap): a STARTED face first resets its slot's identity to (-1, 0); then
 * idx[i] >= 0 && score[i] > ident_score makes (idx[i], score[i]) the slot's identity (the best score over the track's life, the earlier one on
 * ties).  A STARTED face without a row still resets its slot.  Outputs ident_idx_dev int32 [B,cap] / ident_score_dev float [B,cap]: a tracked
 * detection gets its slot's identity as it stands after its frame's rows; an untracked one its own row's (idx, score) if it has a row;
 * everything else (-1, 0).  The identity words of the state belong to this call: between a step and its identify they read as they were
 * before the step; afterwards a free slot's are 0.
 *
 * fid_tracker_reset: stream >= 0 frees that stream's slots and zeroes its next_id / lost (refused while a step is pending); -1 does so for
 * every stream and drops a pending step.  fid_tracker_read (synchronises; tests and debugging): slots_host int32 [S,T,FID_TRACK_SLOT_WORDS] =
 * id, missed, since, ident_idx, bits of ident_score, bits of box x1 y1 x2 y2, 0 (reserved); streams_host int32 [S,2] = {next_id, lost}.
 * FID_E_INVALID, nothing enqueued, outputs untouched: a NULL pointer, S < 1, T outside [1, FID_TRACK_MAX_SLOTS], B <= 0, cap <= 0, B * cap not
 * fitting int32, row_cap <= 0, iou_thresh NaN or outside [0, 1), max_age < 0, refresh or retry < 1, a stream[b] >= S, n_rows < 0 or > row_cap,
 * sizes or a stream array that differ from the pending step's.  Both calls are asynchronous on the context's stream and never synchronise
 * with the host, except once when a step's B outgrows the tracker's per-frame table (1024 frames at first). */
typedef struct fid_tracker fid_tracker;
typedef struct fid_track_config {
    float iou_thresh;              /* [0, 1) */
    int32_t max_age, refresh, retry;
} fid_track_config;
#define FID_TRACK_MAX_SLOTS 64
#define FID_TRACK_SLOT_WORDS 10
#define FID_TRACK_STARTED (1 << 8)
#define FID_TRACK_EMBED (1 << 9)
int fid_tracker_create(fid_ctx *ctx, int S, int T, fid_tracker **out);
int fid_tracker_destroy(fid_ctx *ctx, fid_tracker *trk);
int fid_tracker_reset(fid_ctx *ctx, fid_tracker *trk, int stream);
int fid_tracker_read(fid_ctx *ctx, fid_tracker *trk, int32_t *slots_host, int32_t *streams_host);
int fid_track_step(fid_ctx *ctx, fid_tracker *trk, const float *det_dev, const int32_t *counts_dev, const int32_t *stream, int B, int cap,
                   const fid_track_config *cfg, int32_t *track_dev, int32_t *offsets_dev, int32_t *src_dev, int row_cap);
int fid_track_identify(fid_ctx *ctx, fid_tracker *trk, const int32_t *counts_dev, const int32_t *stream, int B, int cap,
                       const int32_t *track_dev, const int32_t *offsets_dev, const int32_t *src_dev, int row_cap, const int32_t *idx_dev,
                       const float *score_dev, int n_rows, int32_t *ident_idx_dev, float *ident_score_dev);

/* ---- coasting: a track's box in the frames where the detector missed it (no reference analogue: the reference draws what it detects,
 * main.py:130-148, so a face the detector drops for three frames is shown in the clear for three frames).  A coaster follows a tracker on the
 * device: for every frame of a step it emits the tracks that are alive but unmatched in that frame -- at their last box, optionally moved
 * along their last velocity and grown per missed frame -- behind the frame's detections, in tables that fid_draw_faces* / fid_redact_faces*
 * read unchanged in the slot form.  It changes nothing the tracker decides; fid_track_step never sees a prediction.
 *
 * State: S x T entries in device memory, owned by the handle, int32 x FID_COAST_WORDS each:
 *   0 id (-1: free, then every other word is 0)   1 missed (frames since the last match)   2 has_vel   3 ident_idx   4 bits of ident_score
 *   5 .. 8 bits of box x1 y1 x2 y2 (the last matched detection)   9 .. 12 bits of vel (per-frame deltas of x1 y1 x2 y2)   13 bits of conf
 *   14, 15  0 (reserved).
 * Config: hold in [0, 1023], the missed frames that are bridged; predict (0 / not 0); grow in [0, 0.5], not NaN; reserved 0.
 *
 * fid_track_coast follows one completed step, i.e. a step after its fid_track_identify (and after fid_track_keep, if any), with the step's
 * stream, B, cap, det, counts, track and optionally fid_track_identify's ident_idx / ident_score [B,cap] (NULL together: every identity is
 * (-1, 0)).  All fp32, every operation rounded on its own, the divide correctly rounded, no FMA.  Per stream, over its frames in batch order
 * (stream[b] < 0 skips the frame), k_b = min(max(counts[b], 0), cap):
 *   detections f = 0 .. k_b - 1.  A detection is TRACKED when its word track[b,f,1] >= 0, its id track[b,f,0] >= 0 and its slot s = word & 0xFF
 *     is < T; any other detection touches no entry.  If a (malformed) track table names one slot twice in a frame, only the higher f is
 *     applied.  The applied detection, against entry[s]:
 *       continues   entry.id == id and the word has no FID_TRACK_STARTED:  d = (float)(missed + 1), vel_k = (det_k - box_k) / d for the four
 *                   coordinates, has_vel = 1.  (After a gap the velocity is the mean over the gap.)
 *       new         otherwise -- another id, or a track that STARTS under the same id, as after fid_tracker_reset --: id, vel = 0, has_vel = 0.
 *       both        box = det[0..3], conf = det[4], missed = 0, (ident_idx, ident_score) = the detection's entries of the identity arrays.
 *   end of frame: every entry with id >= 0 that took no detection in this frame gets missed = min(missed + 1, 1 << 20).  If
 *     1 <= missed <= hold it COASTS in this frame:  m = (float)missed;  p_k = box_k + (vel_k * m) when predict && has_vel (the product is
 *     rounded, then added), else p_k = box_k;  with grow != 0:  g = grow * m, dx = g * (p_x2 - p_x1), dy = g * (p_y2 - p_y1), the emitted box
 *     is (p_x1 - dx, p_y1 - dy, p_x2 + dx, p_y2 + dy);  with grow == 0 the emitted box is p itself, so that without prediction it is the
 *     last box bit for bit.  An entry past hold stays remembered (a later match resumes it, with the velocity over the long gap) but emits
 *     nothing.  An entry ends only when another track takes its slot, or on fid_coaster_reset.
 *   NaN: every float the call stores in the state or emits for a coasting entry -- box, vel, conf, ident_score -- is stored with a NaN
 *     replaced by the quiet NaN 0x7FC00000 (fid_shot_score's rule: hosts and devices disagree on sign and payload).  The detections' own rows
 *     are copied, not computed: they keep their bytes.
 * Outputs (device), cap2 = cap + T: det_out float [B,cap2,5], counts_out int32 [B], track_out int32 [B,cap2,2], idx_out int32 [B,cap2],
 * score_out float [B,cap2].  A frame of a live stream: first its k_b detections, copied verbatim from det, track, ident_idx and ident_score
 * ((-1, 0) without identity arrays); then the entries that coast in this frame in ascending slot order: det row = (emitted box, conf), track =
 * {id, slot | FID_TRACK_COASTED | (missed << 16)}, idx and score = the entry's identity, i.e. the track's as of its last matched frame;
 * counts_out[b] = k_b + c_b; every row behind gets the fillers: det zeros, track {-1,-1}, idx -1, score 0.  A skipped frame has count 0 and
 * only fillers.  Every byte of every output is defined.  The tables are fid_draw_faces* / fid_redact_faces*'s slot form with
 * cap = id_stride = cap2: a named person coasts in the clear under the default redaction, a stranger behind the mosaic, and a coasted
 * region, standing behind the detections, wins where it overlaps one (the highest-index rule).
 * fid_coaster_reset: stream >= 0 frees that stream's entries, -1 all.  fid_coaster_read (synchronises; tests and debugging): entries_host
 * int32 [S,T,FID_COAST_WORDS].
 * FID_E_INVALID, nothing enqueued, outputs and state untouched: a NULL pointer (the two identity inputs may be NULL together, not one of
 * them); S or T outside the tracker's ranges or different from the tracker's; B, cap or a stream array that differ from the tracker's last
 * step's; B * cap2 not fitting int32; a tracker that has run no step, or whose step still waits for its identify; a second coast for the same
 * step (the tracker counts its steps; skipping a step is allowed: the skipped frames do not age the entries); a bad config; a reset of a
 * stream outside [-1, S).  fid_track_coast is asynchronous on the context's stream and never reads back; it synchronises only when B * T
 * outgrows the context's scratch.
 * fid_track_coast_host: the same walk in plain loops on HOST arrays, no device and no tracker involved (entries int32 [S,T,FID_COAST_WORDS] is
 * the caller's, updated in place; a fresh state is id -1, every other word 0): the definition the kernels are tested against.  It refuses
 * what can be checked without a tracker: NULL pointers, S < 1, T outside [1, 64], B or cap <= 0, B * cap2 overflow, a stream[b] >= S, a bad
 * config. */
typedef struct fid_coaster fid_coaster;
typedef struct fid_coast_config {
    int32_t hold;                  /* [0, 1023] */
    int32_t predict;
    float grow;                    /* [0, 0.5] */
    int32_t reserved;              /* 0 */
} fid_coast_config;
#define FID_COAST_WORDS 16
#define FID_TRACK_COASTED (1 << 10)
int fid_coaster_create(fid_ctx *ctx, int S, int T, fid_coaster **out);
int fid_coaster_destroy(fid_ctx *ctx, fid_coaster *coaster);
int fid_coaster_reset(fid_ctx *ctx, fid_coaster *coaster, int stream);
int fid_coaster_read(fid_ctx *ctx, fid_coaster *coaster, int32_t *entries_host);
int fid_track_coast(fid_ctx *ctx, fid_coaster *coaster, fid_tracker *trk, const int32_t *stream, int B, int cap, const float *det_dev,
                    const int32_t *counts_dev, const int32_t *track_dev, const int32_t *ident_idx_dev, const float *ident_score_dev,
                    const fid_coast_config *cfg, float *det_out, int32_t *counts_out, int32_t *track_out, int32_t *idx_out, float *score_out);
int fid_track_coast_host(int32_t *entries, int S, int T, const int32_t *stream, int B, int cap, const float *det, const int32_t *counts,
                         const int32_t *track, const int32_t *ident_idx, const float *ident_score, const fid_coast_config *cfg,
                         float *det_out, int32_t *counts_out, int32_t *track_out, int32_t *idx_out, float *score_out);

/* ---- re-linking: a returning face gets its earlier track's PERSON ID by embedding (no reference analogue: the reference re-identifies against
 * a gallery of names only, so a stranger who walks behind a pillar for longer than max_age frames comes back as somebody new).  A relinker
 * follows a tracker on the device: it keeps the latest embedding of every live track and, per stream, a small pool of recently ended tracks;
 * when a new track gets its first embedding and that embedding scores above a threshold against a pooled one, the new track inherits the old
 * track's person id.  A person id is the id of the first track of a chain; its namespace is the stream's track ids.  Streams never share
 * anything.  It changes nothing the tracker decides; fid_track_step never sees a person id.
 *
 * A relinker belongs to a tracker's shape: S streams x T slots, a pool of L entries per stream (1 <= L <= FID_RELINK_MAX_POOL), embeddings of
 * dim fp16 values, dim >= 8 and a multiple of 8.  State, all in device memory, owned by the handle:
 *   live table, int32 [S,T,FID_RELINK_WORDS]:  0 track id (-1: empty, then every other word is 0)   1 person id   2 has_q   3 bits of the link
 *     score (0: never linked)   4 seen, the frame number of the track's latest row   5 missed   6 the track id it was linked from (-1: none)
 *     7 0;  plus live_q fp16 [S,T,dim].
 *   pool, int32 [S,L,FID_RELINK_WORDS]:  0 person id (-1: free, then every other word is 0)   1 the ended track's id   2 its seen   3 .. 7  0;
 *     plus pool_q fp16 [S,L,dim].
 *   a frame counter per stream: the non-skipped frames since create or reset, 0-based, as the keeper's.
 *   The q row of an empty live entry or a free pool entry is whatever it last held (zeros after create or reset).
 * Config: thresh finite in [0, 1); window >= 0, the frames a pooled track waits; max_age >= 0, which must be the tracker's.
 *
 * fid_track_relink follows one completed step, i.e. a step after its fid_track_identify; its order relative to fid_track_keep and
 * fid_track_coast is free; at most once per step (the tracker's serial decides, as for the keeper).  It takes the step's stream, B, cap,
 * counts, track, offsets, src, row_cap, n_rows and the unit rows q_dev fp16 [n_rows,dim].  A detection is TRACKED when its word
 * track[b,f,1] >= 0, its id t = track[b,f,0] >= 0 and its slot = word & 63 is < T.  Per stream s, over its frames b in batch order
 * (stream[b] < 0: the frame is skipped without ageing and gets {-1,-1} everywhere), n = the stream's frame number,
 * k_b = min(max(counts[b], 0), cap):
 *   0. expiry.  A pool entry with n - seen > window becomes free.
 *   1. sightings.  Tracked detections f = 0 .. k_b - 1 in order.  If the slot's live entry is empty, holds another id, or the word carries
 *      FID_TRACK_STARTED: a non-empty old entry RETIRES, and the entry BEGINS: id = person = t, has_q = 0, link score 0, seen 0, missed 0,
 *      linked-from -1.  The slot counts as seen in this frame and missed = 0.
 *   2. rows.  i in [max(offsets[b], 0), min(offsets[b+1], n_rows, row_cap)) in table order, where src[i] is a tracked detection of this frame
 *      (b * cap <= src[i] < b * cap + k_b); other rows are ignored.  The row acts on its slot's live entry.  If has_q == 0 the row is scored
 *      against every non-free pool entry of s: the fp32 sum over dim of the fp16 products (exact in fp32; the summation order is free).  The
 *      best is the maximum score, the lowest pool index among equals; a NaN is never best.  If best > thresh (strict): person = the entry's
 *      person, linked-from = its track id, the link score is stored and the pool entry becomes free -- a pooled track is claimed once.  In
 *      every case live_q = the row, has_q = 1, seen = n.
 *   3. output, person_dev int32 [B,cap,2]: a tracked detection gets {its slot's live person, word | (FID_TRACK_RELINKED if that person differs
 *      from the live id)}; everything else {-1,-1}.  Every byte is defined.
 *   4. ageing, slots ascending.  A non-empty live entry that was not seen in this frame gets missed += 1; if missed > max_age it retires and
 *      the entry becomes empty.
 *   RETIRE: an entry with has_q == 0 just vanishes.  Otherwise it goes into the lowest free pool index; with no free index it overwrites
 *      the entry with the smallest seen, the lowest index among equals.  It goes in as (person, id, seen, q).
 * With the tracker's max_age, steps 1 and 4 mirror the tracker's own slot life exactly: after any step live word 0 equals
 * fid_tracker_read's slot ids.  The result does not depend on how frames are split into calls, as long as row_cap cuts no row.
 * fid_relinker_reset: stream >= 0 gives that stream the fresh state (empty live entries, a free pool, zero q rows, frame 0), -1 all.
 * fid_relinker_read (synchronises; tests and debugging): live_host int32 [S,T,8], pool_host int32 [S,L,8], frames_host int32 [S] and, where
 * not NULL, live_q_host fp16 [S,T,dim], pool_q_host fp16 [S,L,dim].
 * FID_E_INVALID, nothing enqueued, state and outputs untouched: a NULL pointer; a shape outside the ranges above or different from the
 * tracker's; thresh not finite or outside [0, 1); window < 0 or max_age < 0; n_rows outside [0, row_cap]; B, cap, row_cap or a stream array
 * that differ from the tracker's last step's; a tracker that has run no step, or whose step still waits for its identify; a second relink for
 * one step; a reset of a stream outside [-1, S).  fid_track_relink is asynchronous on the context's stream, one launch, never reads back and
 * allocates nothing.
 * fid_track_relink_host: the same walk in plain loops on HOST arrays, no device and no tracker involved (the five state arrays are the
 * caller's, updated in place; a fresh state is word 0 = -1, everything else 0); it sums ascending.  It refuses what can be checked without a
 * tracker. */
typedef struct fid_relinker fid_relinker;
typedef struct fid_relink_config {
    float thresh;                  /* [0, 1) */
    int32_t window;                /* >= 0 */
    int32_t max_age;               /* >= 0: the tracker's */
} fid_relink_config;
#define FID_RELINK_WORDS 8
#define FID_RELINK_MAX_POOL 64
#define FID_TRACK_RELINKED (1 << 11)
int fid_relinker_create(fid_ctx *ctx, int S, int T, int L, int dim, fid_relinker **out);
int fid_relinker_destroy(fid_ctx *ctx, fid_relinker *relinker);
int fid_relinker_reset(fid_ctx *ctx, fid_relinker *relinker, int stream);
int fid_relinker_read(fid_ctx *ctx, fid_relinker *relinker, int32_t *live_host, int32_t *pool_host, int32_t *frames_host, uint16_t *live_q_host,
                      uint16_t *pool_q_host);
int fid_track_relink(fid_ctx *ctx, fid_relinker *relinker, fid_tracker *trk, const int32_t *stream, int B, int cap, const int32_t *counts_dev,
                     const int32_t *track_dev, const int32_t *offsets_dev, const int32_t *src_dev, int row_cap, int n_rows, const uint16_t *q_dev,
                     const fid_relink_config *cfg, int32_t *person_dev);
int fid_track_relink_host(int32_t *live, uint16_t *live_q, int32_t *pool, uint16_t *pool_q, int32_t *frames, int S, int T, int L, int dim,
                          const int32_t *stream, int B, int cap, const int32_t *counts, const int32_t *track, const int32_t *offsets,
                          const int32_t *src, int row_cap, int n_rows, const uint16_t *q, const fid_relink_config *cfg, int32_t *person);

/* ---- drawing detections, names and scores onto the frames (reference main.py:130-148 with utils/helpers.py:126-179 draw_bbox / draw_bbox_info):
 * the overlay of a whole batch in place on the device, enqueued behind the match with nothing read back first.  OpenCV's thick-line caps and
 * Hershey font are NOT reproduced; taken from the reference are the integer truncation of the box, the corner length, the
 * bar rectangle, the text anchor, the label string and its two decimals, the unknown colour and the draw order.  The raster rules:
 *
 * One face, from its det row (x1f, y1f, x2f, y2f, conf), an identity (idx, score), an optional track id, the label table and the style:
 *   x1, y1, x2, y2 = the floats truncated toward zero; w = x2 - x1, h = y2 - y1.  The face draws nothing unless all four floats are finite,
 *   each |v| < 2^23, and w > 0 && h > 0.  Known = 0 <= idx < G with a label table: the colour is the table's BGR, else style.unknown_bgr.
 *   L = (int)(proportion * (double)min(w, h));  r = (thickness - 1) / 2;  s = score if finite and > 0, else 0;
 *   bh = (int)(s * (float)h) in fp32;  cents = min((int)rint((double)s * 100.0), 999) (ties to even: Python's f"{np.float32(s):.2f}").
 *   Text of a known face: "#<id> " (only with FID_DRAW_TRACK_ID and a track id >= 0), the name (at most FID_LABEL_MAX bytes, a byte outside
 *   0x20..0x7E drawn as '?'), ": ", cents / 100, '.', two digits.  Of an unknown face: "#<id>" under the same condition, else none.
 *   Pixel set, clipped to the frame, all in the face's colour:
 *     outline   x1 <= x <= x2 on rows y1 and y2, y1 <= y <= y2 on columns x1 and x2;
 *     arms      per corner (cx, cy, sx, sy) the segments cx .. cx + sx * L on row cy and cy .. cy + sy * L on column cx, inclusive, every point
 *               of a segment stamping a thickness x thickness square;
 *     bar       (known faces, style.bar) x2 + 10 <= x <= x2 + 20, y2 - bh <= y <= y2;
 *     text      (style.text_scale = t > 0) character k has its left edge at X = x1 + 6 * t * k and the bottom row of its cell at Y = y1 - 10; the
 *               5 x 7 glyph (fid_draw_glyphs: 95 x 7 bytes for ASCII 0x20..0x7E, top row first, bit 4 = leftmost column) is magnified t
 *               times: (x, y) is lit iff the glyph bit at column (x - X) / t, row 6 - (Y - y) / t is set.
 * One frame: a pixel takes the colour of the HIGHEST face index whose set contains it (the reference draws the faces in detection order); a
 * pixel in no set is not written, and nothing is ever read from the frame.
 *
 * fid_labels: per gallery row the name bytes and a BGR colour, device resident.  names: the rows' bytes back to back, row g =
 * names[name_offsets[g] .. name_offsets[g+1]); bgr [G,3] or NULL: row g gets h = (uint32_t)(g + 1) * 2654435761u -> (h >> 24, (h >> 16) & 255,
 * (h >> 8) & 255) (the reference picks them at random, main.py:160).  fid_labels_create synchronises (one copy); G <= 0 or offsets that
 * decrease are FID_E_INVALID.
 *
 * fid_draw_faces: frames_dev uint8 [B,H,W,3] drawn IN PLACE (a caller that still needs the clean frames draws after their last reader);
 * det_dev [B,cap,5] / counts_dev [B] as fid_scrfd_postprocess* writes them.  Three identity forms:
 *   idx_dev == NULL      detections only: n_b = min(max(counts[b], 0), cap), every face unknown;
 *   offsets_dev == NULL  slots: face (b, f) reads idx / score[b * id_stride + f], n_b = min(max(counts[b], 0), cap, id_stride) (a pipeline's
 *                        B x F slots: id_stride = F; fid_track_identify's ident_idx / ident_score: id_stride = cap);
 *   offsets_dev != NULL  rows in fid_face_pack's format: face f of frame b is row offsets[b] + f,
 *                        n_b = clamp(min(offsets[b+1], n_rows) - offsets[b], 0, cap) (a negative offsets[b]: no face).
 * track_dev: optional int32 [B,cap,2] as fid_track_step writes it (word 0 is the id).  labels may be NULL: no names, every face unknown.
 * FID_E_INVALID, nothing enqueued, the frames untouched: a NULL ctx, frames, det, counts or style; B, H, W or cap <= 0; B * cap or H * W * 3
 * not fitting int32; thickness even or outside 1 .. 15; text_scale outside 0 .. 4; proportion NaN or outside [0, 1]; idx without score;
 * id_stride <= 0 in the slot form; n_rows < 0.  Asynchronous on the context's stream; it never synchronises with the host, except once when
 * B * cap outgrows the context's scratch.
 *
 * fid_draw_faces_host: the same records and the same coverage test in plain loops on HOST arrays, no device involved: the definition the
 * device kernels are tested against, and what utils/helpers.draw_bbox / draw_bbox_info / draw_faces call.  The label table is given as the
 * arguments of fid_labels_create (name_offsets NULL: none).
 *
 * fid_draw_faces_nv12: the same overlay IN PLACE on NV12 frames (nv12_dev, desc: the layout of the NV12 section above), so that an annotated
 * video leaves the device at 1.5 bytes per pixel and no BGR frame is ever built.  Face records, label text, pixel sets, draw order and the
 * three identity forms are fid_draw_faces' own; what is defined here is how a pixel set lands on two planes, with the forward table of the
 * layout's standard (fid_bgr_to_nv12):
 *   Y plane    a pixel in some face's set gets Y(colour) of the HIGHEST face index whose set contains it; every other pixel is not written
 *              (the pixels fid_draw_faces writes, exactly);
 *   UV plane   a pair is written when at least one of the four pixels of its 2 x 2 group is in some set, and gets (U, V)(colour) -- the flat
 *              group S = 4 * colour -- of the HIGHEST face index whose set contains ANY of the four; every other pair is not written.
 * A chroma sample cannot be shared out among faces, so a thin line colours the whole pair it touches: the uncovered pixels of a partly
 * covered group keep their luma and take the line's chroma.  Nothing is read from the frames; padding (between W and pitch, between the
 * planes, behind the last UV row, between the frames) is never written.  FID_E_INVALID, nothing enqueued, the frames untouched: everything
 * fid_draw_faces refuses, and a layout fid_nv12_check refuses (NULL, odd H or W, pitch < W, overlapping planes or frames, unknown standard).
 * fid_draw_faces_nv12_host: the same in plain loops on HOST arrays: the faces in ascending order, each covered pixel sets its Y and the pair
 * of its group. */
typedef struct fid_labels fid_labels;
typedef struct fid_draw_style {
    double proportion;             /* corner length / min(w, h), [0, 1]; a double: the reference multiplies by the Python float 0.2 */
    int32_t thickness;             /* of the corner arms: odd, 1 .. 15 */
    int32_t text_scale;            /* 0: no text; 1 .. 4 */
    int32_t bar;                   /* non-zero: the similarity bar of known faces */
    int32_t flags;                 /* FID_DRAW_TRACK_ID */
    uint8_t unknown_bgr[4];        /* colour of an unknown face (byte 3 unused) */
} fid_draw_style;
#define FID_LABEL_MAX 32
#define FID_DRAW_TRACK_ID 1
int fid_labels_create(fid_ctx *ctx, const char *names, const int32_t *name_offsets, const uint8_t *bgr, int G, fid_labels **out);
int fid_labels_destroy(fid_ctx *ctx, fid_labels *labels);
int fid_draw_faces(fid_ctx *ctx, uint8_t *frames_dev, int B, int H, int W, const float *det_dev, const int32_t *counts_dev, int cap,
                   const int32_t *idx_dev, const float *score_dev, int id_stride, const int32_t *offsets_dev, int n_rows,
                   const int32_t *track_dev, fid_labels *labels, const fid_draw_style *style);
int fid_draw_faces_host(uint8_t *frames, int B, int H, int W, const float *det, const int32_t *counts, int cap, const int32_t *idx,
                        const float *score, int id_stride, const int32_t *offsets, int n_rows, const int32_t *track, const char *names,
                        const int32_t *name_offsets, const uint8_t *bgr, int G, const fid_draw_style *style);
int fid_draw_faces_nv12(fid_ctx *ctx, uint8_t *nv12_dev, const fid_nv12_desc *desc, int B, int H, int W, const float *det_dev,
                        const int32_t *counts_dev, int cap, const int32_t *idx_dev, const float *score_dev, int id_stride,
                        const int32_t *offsets_dev, int n_rows, const int32_t *track_dev, fid_labels *labels, const fid_draw_style *style);
int fid_draw_faces_nv12_host(uint8_t *nv12, const fid_nv12_desc *desc, int B, int H, int W, const float *det, const int32_t *counts, int cap,
                             const int32_t *idx, const float *score, int id_stride, const int32_t *offsets, int n_rows, const int32_t *track,
                             const char *names, const int32_t *name_offsets, const uint8_t *bgr, int G, const fid_draw_style *style);
int fid_draw_glyphs(uint8_t *out /* [95 * 7] */);

/* ---- redacting faces on the frames: a mosaic or a solid fill over every selected face of a whole batch, in place on the device, enqueued
 * behind the match with nothing read back first -- so that the video fid_draw_faces annotates may leave the box without showing passers-by.
 * Nothing here is the reference's.  Integer arithmetic throughout; the device, the host twins and a numpy restatement agree to the byte.
 *
 * Faces.  The face count per frame and the three identity forms (idx == NULL; slots with id_stride; rows with offsets / n_rows) are
 *   fid_draw_faces' own.  A face is KNOWN iff an idx array is given and its entry is >= 0 (no label table is involved); with idx == NULL every
 *   face is unknown.  A face is SELECTED iff style.who has the bit of its class.  score is accepted and ignored (it keeps the argument shape).
 * Box.  x1, y1, x2, y2 = the floats truncated toward zero; the face is skipped unless all four are finite, each |v| < 2^23, and
 *   w = x2 - x1 > 0 && h = y2 - y1 > 0.
 * Region, aligned on both axes to the 2 x 2 chroma grid so that BGR and NV12 share one geometry:
 *   mx = (int)(expand * (double)w), my = (int)(expand * (double)h);
 *   rx0 = x1 - mx rounded DOWN to even (floor, also for negatives), rx1 = (x2 + mx) | 1; ry0, ry1 likewise;
 *   the region is the inclusive rectangle [rx0, rx1] x [ry0, ry1] intersected with the frame.
 * Cells.  s = max(w, h); c = max(2, s / cells rounded UP to even) (integer division).  Cell (i, j) is
 *   [rx0 + i*c, rx0 + (i+1)*c - 1] x [ry0 + j*c, ry0 + (j+1)*c - 1] intersected with the region and the frame: the grid is anchored at the
 *   UNCLIPPED rx0, ry0, so it moves with the face and not with the frame edge.
 * Values, MOSAIC.  BGR: per channel (sum + n / 2) / n over the n pixels of the clipped cell -- integer division, half rounds up; the sum is
 *   exact for every frame the call accepts (it can pass 2^32).  NV12: Y the same mean over the cell's Y bytes, U and V each the same mean over
 *   the cell's chroma pairs (H and W are even, region and cells even-aligned with an even size: every 2 x 2 group lies wholly inside or
 *   outside a region, and inside one cell).  Nothing is converted: the BGR and the NV12 result are defined separately.
 * Values, FILL.  BGR: fill_bgr.  NV12: Y(fill_bgr) and the (U, V) of the flat group 4 * fill_bgr with the layout's forward table, as
 *   fid_draw_faces_nv12 colours a pixel.
 * Several faces.  Every mean is taken from the frame AS IT WAS BEFORE THE CALL; a pixel (or an NV12 group) inside several selected regions
 *   takes the value of the HIGHEST face index whose clipped region contains it (the overlay's order).  The result depends on no schedule.
 *   Applying the call twice gives the first result again in every frame whose selected regions do not overlap, and under FILL always (a
 *   cell of constant v has mean v); a cell partly under a higher face holds two values after the first call, and its mean moves.
 * Written: only pixels inside a selected, clipped region.  NV12 padding (between W and pitch, between the planes, behind the last UV row,
 *   between the frames) is never read or written.
 *
 * FID_E_INVALID, nothing enqueued, the frames untouched: everything fid_draw_faces refuses for the shared arguments (a NULL ctx, frames, det
 * or counts; B, H, W or cap <= 0; B * cap or H * W * 3 not fitting int32; idx without score; id_stride <= 0 in the slot form; n_rows < 0); a
 * NULL style, an unknown mode, who outside 1 .. 3, cells outside 1 .. 16, expand NaN or outside [0, 0.5], reserved != 0; for NV12 whatever
 * fid_nv12_check refuses.  Asynchronous on the context's stream; never synchronises with the host, except once when the scratch is outgrown.
 * The scratch holds, per face slot, a record, a 16-byte extent and a cell table of
 *   (floor(1.5 * (1 + 2 * expand) * cells) + 3)^2 entries of 4 bytes (MOSAIC only)
 * -- the most cells one face can have (derived in csrc/redact_core.h): 289 at the defaults, 2601 at cells = 16, expand = 0.5.
 *
 * Redaction destroys pixels: call it after the step's last reader of the clean frames (the warp, fid_face_measure, the best-shot crops), and
 * before fid_draw_faces if boxes and names are to stay legible on top.  A mosaic is obfuscation, not cryptography; FILL is the strong mode.
 * fid_redact_faces_host / fid_redact_faces_nv12_host: the same in plain loops on HOST arrays, no device involved: the table of cell values
 * first, the writes second. */
#define FID_REDACT_MOSAIC 0
#define FID_REDACT_FILL 1
#define FID_REDACT_UNKNOWN 1
#define FID_REDACT_KNOWN 2
typedef struct fid_redact_style {
    int32_t mode;          /* FID_REDACT_MOSAIC 0 | FID_REDACT_FILL 1 */
    int32_t who;           /* bit 0 FID_REDACT_UNKNOWN, bit 1 FID_REDACT_KNOWN; 0 is FID_E_INVALID */
    int32_t cells;         /* mosaic cells along the LONGER side of the box, 1 .. 16 */
    int32_t reserved;      /* 0 */
    double  expand;        /* margin as a share of w and of h, [0, 0.5] */
    uint8_t fill_bgr[4];   /* FILL colour (byte 3 unused) */
} fid_redact_style;
int fid_redact_faces(fid_ctx *ctx, uint8_t *frames_dev, int B, int H, int W, const float *det_dev, const int32_t *counts_dev, int cap,
                     const int32_t *idx_dev, const float *score_dev, int id_stride, const int32_t *offsets_dev, int n_rows,
                     const fid_redact_style *style);
int fid_redact_faces_host(uint8_t *frames, int B, int H, int W, const float *det, const int32_t *counts, int cap, const int32_t *idx,
                          const float *score, int id_stride, const int32_t *offsets, int n_rows, const fid_redact_style *style);
int fid_redact_faces_nv12(fid_ctx *ctx, uint8_t *nv12_dev, const fid_nv12_desc *desc, int B, int H, int W, const float *det_dev,
                          const int32_t *counts_dev, int cap, const int32_t *idx_dev, const float *score_dev, int id_stride,
                          const int32_t *offsets_dev, int n_rows, const fid_redact_style *style);
int fid_redact_faces_nv12_host(uint8_t *nv12, const fid_nv12_desc *desc, int B, int H, int W, const float *det, const int32_t *counts, int cap,
                               const int32_t *idx, const float *score, int id_stride, const int32_t *offsets, int n_rows,
                               const fid_redact_style *style);

/* ---- face gates of the reference's product layer: replaces smart_face_recognition.py:1145-1216
 * (assess_face_quality), :1218-1297 (get_face_pose_angles / is_side_face), :1299-1399 (analyze_bbox_for_side_face) and the
 * best-face selection with its four rejections (:1473-1519), for every face of a batch in one launch on the post-process's own
 * device arrays.  The thresholds are the reference's config.json blocks face_quality / side_face_detection / face_detection. */
typedef struct fid_gate_config {
    float size_normalization;
    float w_detection, w_size, w_blur, w_pose, w_lighting;
    float ar_extreme_profile, ar_very_strong_profile, ar_strong_profile, ar_very_wide, ar_wide, ar_moderately_wide;
    float area_extremely_small, area_very_small, area_small, area_very_large, area_large;
    float compactness_very_low, compactness_low;
    float confidence_very_low, confidence_low;
    float edge_position_threshold;
    int32_t decision_threshold;
    float yaw_threshold, pitch_threshold;              /* degrees */
    float confidence_threshold, min_quality_threshold;
} fid_gate_config;
enum { FID_GATE_ACCEPT = 0, FID_GATE_NO_FACE = 1, FID_GATE_LOW_CONFIDENCE = 2, FID_GATE_SIDE_FACE = 3, FID_GATE_LOW_QUALITY = 4 };
/* det [B,cap,5], kps [B,cap,10], counts [B] as fid_scrfd_postprocess writes them; the first min(counts[b], faces_per_frame) slots
 * of frame b are faces.  pose (optional, may be NULL): FLOAT64 [B, faces_per_frame, 2] yaw / pitch in radians (the reference hands python floats to
 * math.degrees, :1226-1240: float32 here would move the verdict of an angle at the threshold), 0 = not available (then the
 * bbox analysis decides, as in the reference).  Outputs (device): quality [B, faces_per_frame, 5] = overall, blur, pose, lighting,
 * size (zeros in empty slots); side [B, faces_per_frame] = analyze_bbox_for_side_face's score | is_side_face << 16; best [B, 2] =
 * index of the FIRST face with the highest det_score (-1: no face) and its verdict (FID_GATE_*), checked in the reference's
 * order: confidence_threshold, side face, min_quality_threshold. */
int fid_face_gates(fid_ctx *ctx, const float *det_dev, const float *kps_dev, const int32_t *counts_dev, int B, int cap,
                   int faces_per_frame, const double *pose_dev, const fid_gate_config *cfg, float *quality_dev,
                   int32_t *side_dev, int32_t *best_dev);

/* ---- measured face quality: sharpness, exposure and pose of every aligned crop, on the device.  (No reference analogue: assess_face_quality,
 * smart_face_recognition.py:1145-1216, sets blur = min(1, det_score * 1.2) and lighting = min(1, det_score * 1.1) without reading a pixel, and
 * is_side_face reads face.yaw / face.pitch, which SCRFD never provides.)  Opt-in: nothing calls these unless asked to.
 *
 * fid_face_measure: one launch over a table of crops.  crops_dev uint8 [n_rows,112,112,3] BGR as fid_align_crops* writes them.  src_dev (may be
 * NULL) is the row table of fid_face_pack / fid_track_step: a row with src[i] < 0 is no face, its crop bytes are ignored and all 16 of its
 * output words are 0; row i reads the landmarks kps[src[i]*10 ..]; with src == NULL every row is a face and reads kps[i*10 ..].  kps_dev and
 * M_dev (row i = the 6 doubles fid_align_crops* writes) may both be NULL: then only the pixel part is computed.
 * Pixel part, all integer, so independent of the order of summation:
 *   Y = (29*B + 150*G + 77*R + 128) >> 8;  window = the 80 x 80 pixels with 16 <= x, y < 96 (N = 6400: it holds all five template landmarks and
 *   leaves out most background and most of the warp's zero border);  L = 4*Y(x,y) - Y(x-1,y) - Y(x+1,y) - Y(x,y-1) - Y(x,y+1) on every window
 *   pixel, neighbours at coordinate 15 and 96 read from the crop.
 *   stats int64 [n_rows,8] = N, sum Y, sum Y^2, sum L, sum L^2, n_dark (Y <= 16), n_bright (Y >= 239), flags (bit 0: pixel part valid, bit 1:
 *   pose part valid).
 * measure float [n_rows,8], each word computed in fp64 from the integers -- the integer expression in int64, converted once to double, one
 * correctly rounded divide (and square root) -- and rounded once to fp32:
 *   0 sharpness = (N*sum L^2 - (sum L)^2) / (N*N)          the variance of the Laplacian
 *   1 mean      = sum Y / N
 *   2 contrast  = sqrt((N*sum Y^2 - (sum Y)^2) / (N*N))
 *   3 clipped   = (n_dark + n_bright) / N
 * Pose part, fp64 with + - * / and square root only, every operation rounded separately, no FMA.  k_i = landmark i widened to double, t_i = the
 * float32 ArcFace template widened to double (as the warp sees it);  p_i.x = (M0*k_i.x + M1*k_i.y) + M2,  p_i.y = (M3*k_i.x + M4*k_i.y) + M5.
 * For a point set q:  ex = (q0.x+q1.x)/2, ey = (q0.y+q1.y)/2, mx = (q3.x+q4.x)/2, my = (q3.y+q4.y)/2, w = q1.x - q0.x, h = my - ey,
 * Ry(q) = (q2.x - (ex+mx)/2) / w,  Rp(q) = (q2.y - ey) / h.
 *   4 yaw      = Ry(p) - Ry(t)     the nose's offset from the face's vertical axis in eye widths; positive: towards +x in the crop
 *   5 pitch    = Rp(p) - Rp(t)
 *   6 residual = sqrt(sum_i((p_i.x-t_i.x)^2 + (p_i.y-t_i.y)^2) / 5)    i = 0 .. 4 left to right: RMS misfit to the template, in crop pixels
 *   7 0
 * The pose part is valid iff landmarks and M are given, all six entries of M are finite, w(p) > 0 and h(p) > 0, and the three fp32 words are
 * finite; otherwise the three words are 0 and flag bit 1 is clear.  Ratios, not angles: no transcendental function, so device, host and a
 * numpy restatement agree to the bit.
 * n_rows == 0 returns FID_OK and enqueues nothing.  FID_E_INVALID: n_rows < 0, a NULL ctx, crops or output pointer, exactly one of kps / M.
 * Asynchronous on the context's stream; it never synchronises with the host.  n_rows is not limited to 65535.
 * fid_face_measure_host: the same definition in plain loops on HOST arrays, no device involved. */
int fid_face_measure(fid_ctx *ctx, const uint8_t *crops_dev, int n_rows, const float *kps_dev, const int32_t *src_dev, const double *M_dev,
                     int64_t *stats_dev, float *measure_dev);
int fid_face_measure_host(const uint8_t *crops, int n_rows, const float *kps, const int32_t *src, const double *M, int64_t *stats,
                          float *measure);
/* fid_face_gates with measured scores.  Same outputs, layouts, best-face rule and verdict order as fid_face_gates; no pose input.  Face f of
 * frame b reads row offsets[b] + f of stats / measure (offsets_dev: fid_face_pack's format, the row form of fid_draw_faces), or row
 * b * faces_per_frame + f when offsets_dev is NULL.  A face whose row is < 0 or >= n_rows gets exactly what fid_face_gates computes for it
 * (n_rows = 0: every face; stats and measure may then be NULL), and so does each part whose flag bit is clear: bit 0 for blur and lighting,
 * bit 1 for pose and the landmark side test.  fp32, one rounded operation each:
 *   blur     = min(1, sharpness / sharpness_normalization)
 *   lighting = min(1, contrast / contrast_normalization) * (1 - clipped)
 *   pose     = max(0, 1 - residual / residual_normalization)
 * size, the detection term and the weighted sum are fid_face_gates'.  Side flag: the bounding-box analysis (score >= decision_threshold), OR
 * |yaw| > yaw_ratio_threshold, OR |pitch| > pitch_ratio_threshold (both strict, fp32).
 * The defaults the Python binding suggests (100, 40, 8 pixels, 0.25, 0.25) are UNCALIBRATED: nobody has measured them on real faces; they are
 * starting points for a user's own calibration. */
typedef struct fid_measure_config {
    float sharpness_normalization, contrast_normalization, residual_normalization;
    float yaw_ratio_threshold, pitch_ratio_threshold;
} fid_measure_config;
int fid_face_gates_measured(fid_ctx *ctx, const float *det_dev, const float *kps_dev, const int32_t *counts_dev, int B, int cap,
                            int faces_per_frame, const int64_t *stats_dev, const float *measure_dev, const int32_t *offsets_dev,
                            int n_rows, const fid_gate_config *cfg, const fid_measure_config *mcfg,
                            float *quality_dev, int32_t *side_dev, int32_t *best_dev);

/* ---- best shots: of the faces a track embeds, keep the best one on the device; hand an ended track out as one finished visit.  (No reference
 * analogue: the reference embeds and matches every face of every frame and forgets; its visits come from files.)  Opt-in: nothing calls
 * these unless asked to.
 *
 * fid_shot_score: one fp32 score per row of fid_face_measure's output, one thread per row.  fp32, every operation rounded on its own, no FMA,
 * correctly rounded divides -- fid_face_gates_measured's three terms from the same fid_measure_config fields (as UNCALIBRATED as they are there):
 *   b = min(1, sharpness / sharpness_normalization)
 *   l = min(1, contrast / contrast_normalization) * (1 - clipped)
 *   p = max(0, 1 - residual / residual_normalization)
 *   score = (b * l) * p        (min / max as `x < 1 ? x : 1` / `x > 0 ? x : 0`; a NaN result is written as the quiet NaN 0x7FC00000)
 * Flags (stats word 7): bit 0 clear (no face, or no valid pixel part): score -1.0f, the row is never a candidate.  Bit 1 clear: p = 0, so the
 * score is 0: still a candidate, but the weakest.  n_rows == 0: FID_OK, nothing enqueued.  FID_E_INVALID: a NULL pointer, n_rows < 0, a
 * normalisation that is not finite and > 0.  fid_shot_score_host: the same function on HOST arrays, no device involved.
 *
 * A keeper (fid_shots) belongs to a tracker's shape: S streams x T slots, embeddings of `dim` fp16 values.  All state is in device memory:
 * the live store (S x T entries: meta, q, and the crop if keep_crops), the finished store (finished_cap entries of the same record, plus
 * count and dropped) and a frame counter per stream.  Meta, int32 x FID_SHOT_META_WORDS:
 *   0 stream   1 track id (-1: an empty entry, then every other word is 0)   2 ident_idx   3 bits of ident_score   4 bits of the shot's score
 *   (-1.0f: the track has had no candidate row yet; then words 5 and 7 .. 11 are 0)   5 frame number of the shot   6 rows of this track seen
 *   so far   7 .. 10 bits of the shot's box   11 bits of its detection score   12 .. 15 0.
 * The frame number is the stream's count of non-skipped frames over all keep calls since create, 0-based.
 *
 * fid_track_keep follows one completed step, i.e. a step after its fid_track_identify, with the step's stream, sizes, track, offsets and src
 * again, any float score[n_rows] (fid_shot_score's or the caller's own), the step's unit fp16 rows q_dev [n_rows,dim], its crops
 * [n_rows,112,112,3] (may be NULL without keep_crops), det_dev [B,cap,5] and optionally fid_track_identify's ident_idx / ident_score [B,cap].
 * Per stream s, over the step's rows i < min(offsets[B], n_rows, row_cap) in table order whose frame b = src[i] / cap has stream[b] == s:
 *   1. a row whose track word is negative is untracked and is skipped.
 *   2. otherwise the row has (slot, id).  If the live entry of (s, slot) holds another id -- or the same id while the row carries
 *      FID_TRACK_STARTED: after fid_tracker_reset a stream's ids begin again at 0 --, that entry FINISHES NOW: it is appended to the
 *      finished store and the entry becomes empty.  An empty entry begins the track: id, ident (-1, 0), score -1.0f, rows 0.
 *   3. rows += 1; with identity arrays, words 2 and 3 become ident_idx / ident_score at src[i]: the track's name as of its latest row,
 *      whichever row is the best shot.
 *   4. the row is a CANDIDATE iff score[i] >= 0 (false for a NaN).  A candidate replaces the entry's shot iff the entry has no shot yet for
 *      this id, or score[i] > the stored score (strict: on a tie the earlier row stays).  A replacement copies score, frame number, box,
 *      detection score, q row and crop.
 *   5. after the stream's rows, slots 0 .. T-1 ascending: a live entry whose id is not the id the tracker's slot holds now finishes (a freed,
 *      reset or reused slot).  This runs for every stream, with or without frames in the step.
 *   6. a track that never had a candidate row finishes without a record.
 * The finished order is streams ascending, within a stream the order above.  With the finished store full the record is dropped and
 * dropped += 1; the live entry is cleared all the same.  Skipping the keep for a step is allowed; the tracks that started and ended unseen
 * leave no record.
 * fid_shots_flush finishes every live entry of the stream in slot order (-1: all streams in stream order): the end of a video.
 * fid_shots_finished (synchronises) reads count and dropped and hands out the finished store's device arrays: meta int32 [finished_cap,16],
 * q fp16 [finished_cap,dim] -- rows 0 .. count-1 are fid_gallery_group's queries where they lie -- crops uint8 [finished_cap,112,112,3] (NULL
 * without keep_crops); each out-pointer may be NULL.  fid_shots_clear_finished sets count and dropped to 0.  fid_shots_read (synchronises; tests
 * and debugging): the live meta, int32 [S,T,16].
 * FID_E_INVALID, nothing enqueued, state untouched: a NULL required pointer; S or T outside the tracker's ranges (and S * 64 * 16 must fit
 * int32) or different from the tracker's; dim < 1; finished_cap < 1; crops_dev == NULL with keep_crops; exactly one of the identity arrays;
 * n_rows outside [0, row_cap]; B, cap, row_cap or a stream array that differ from the tracker's last step's; a tracker that has run no step,
 * or whose step still waits for its identify; a second keep for the same step (the tracker counts its steps; the keeper remembers the last
 * one it saw); a flush of a stream outside [-1, S).
 * fid_track_keep and fid_shots_flush are asynchronous on the context's stream and never synchronise with the host (the keeper's event table
 * grows by allocation alone when n_rows outgrows it, 1024 rows at first). */
typedef struct fid_shots fid_shots;
#define FID_SHOT_META_WORDS 16
int fid_shot_score(fid_ctx *ctx, const int64_t *stats_dev, const float *measure_dev, int n_rows, const fid_measure_config *mcfg,
                   float *score_dev);
int fid_shot_score_host(const int64_t *stats, const float *measure, int n_rows, const fid_measure_config *mcfg, float *score);
int fid_shots_create(fid_ctx *ctx, int S, int T, int dim, int finished_cap, int keep_crops, fid_shots **out);
int fid_shots_destroy(fid_ctx *ctx, fid_shots *shots);
int fid_track_keep(fid_ctx *ctx, fid_shots *shots, fid_tracker *trk, const int32_t *stream, int B, int cap, const int32_t *track_dev,
                   const int32_t *offsets_dev, const int32_t *src_dev, int row_cap, int n_rows, const float *score_dev, const uint16_t *q_dev,
                   const uint8_t *crops_dev, const float *det_dev, const int32_t *ident_idx_dev, const float *ident_score_dev);
int fid_shots_flush(fid_ctx *ctx, fid_shots *shots, int stream);
int fid_shots_finished(fid_ctx *ctx, fid_shots *shots, int32_t *count, int32_t *dropped, const int32_t **meta_dev, const uint16_t **q_dev,
                       const uint8_t **crops_dev);
int fid_shots_clear_finished(fid_ctx *ctx, fid_shots *shots);
int fid_shots_read(fid_ctx *ctx, fid_shots *shots, int32_t *live_meta_host);

/* ---- embeddings -> unit fp16 rows: the norm half of reference utils/helpers.py:120-123 ------
 * A row whose fp32 sum of squares is not in (0, inf) -- all zero, a NaN or inf element, squares that overflow or underflow -- becomes an all +0.0 row. */
int fid_l2_normalize_f16(fid_ctx *ctx, const float *emb_dev, int n, int dim, void *out_f16_dev);
/* the same for the n = B * faces_per_frame face slots of a batch: slot (b, f) with f >= counts[b] holds no face (reference
 * main.py:132 iterates detected faces only) and is written as a zero row, which scores 0 against every gallery row and so never
 * matches (fid_match: idx -1, score 0).  Its FIRST element is -0.0 (fp16 bit pattern 0x8000), every other +0.0: the same numbers, but
 * told apart from the all +0.0 row a degenerate embedding (zero / NaN / inf norm) of a DETECTED face gets.  The unit-embedding matrix
 * thereby carries the face counts exactly: after the all-gather of SURVEY.md 8e every rank can tell another rank's faces from its
 * empty slots (row == {-0.0, +0.0 ...} <=> no face; pipeline.gathered_face_counts). */
int fid_l2_normalize_f16_slots(fid_ctx *ctx, const float *emb_dev, int n, int dim, const int32_t *counts_dev,
                               int faces_per_frame, void *out_f16_dev);

/* the same for the rows of a packed table (fid_face_pack; main.py:130-134, models/scrfd.py:159-177): src[i] < 0 -> the empty-slot marker
 * row (-0.0 then +0.0s); otherwise the arithmetic of fid_l2_normalize_f16 (degenerate embedding -> all +0.0 row). */
int fid_l2_normalize_f16_packed(fid_ctx *ctx, const float *emb_dev, int n_rows, int dim, const int32_t *src_dev,
                                void *out_f16_dev);

/* ---- gallery match: replaces the per-target python loop of reference main.py:136-142 --------
 * gallery: host fp32 [G, dim] raw embeddings (as build_targets collects them, main.py:102-103).
 * fid_match: for every query row (unit fp16) the first index of the maximum cosine, provided
 * it is > max(0, thresh); otherwise idx = -1 and score = 0 (strict '>' like main.py:140). */
int fid_gallery_create(fid_ctx *ctx, const float *gallery, int G, int dim, fid_gallery **out);
int fid_gallery_destroy(fid_ctx *ctx, fid_gallery *g);
int fid_match(fid_ctx *ctx, fid_gallery *g, const void *query_f16_dev, int n, float thresh,
              int32_t *idx_dev, float *score_dev);
int fid_gallery_info(fid_gallery *g, int *G, int *G_padded, int *dim);
/* device address of the unit fp16 rows [G_padded, dim] (read-only view; owned by the gallery) */
int fid_gallery_data(fid_gallery *g, void **unit_rows_dev);
/* Vector-store use of the gallery -- the product layer's QdrantManager (reference qdrant_manager.py:91-212,
 * smart_face_recognition.py:1619-1643): top-k cosine search with a score threshold (k in {1,2,4,5,8};
 * results score-descending, index-ascending on ties, -1/0 beyond the last hit) and in-place upsert / delete
 * of rows (an all-zero embedding deletes: a zero row can never match). */
int fid_gallery_topk(fid_ctx *ctx, fid_gallery *g, const void *query_f16_dev, int n, int k, float thresh,
                     int32_t *idx_dev, float *score_dev);
int fid_gallery_set_rows(fid_ctx *ctx, fid_gallery *g, const int32_t *rows_host, const float *emb_host, int n);
/* Fused top-k search: the contract of fid_gallery_topk for ANY 1 <= k <= FID_TOPK_MAX (`limit` of qdrant_manager.py:138-183 is an arbitrary
 * integer), computed without the n x G score matrix: per query the k best (score, row) pairs, score descending, row ascending among equal
 * scores; only scores strictly > max(0, thresh) count and a query with fewer hits is padded with (-1, 0.0) -- all n x k entries of idx_dev
 * int32 [n, k] and score_dev float [n, k] are always written.  A NaN score, a zero (deleted / free) row and a padding row >= G are never reported.
 * It IS fid_topk_keys(first_row = 0) followed by fid_topk_merge(parts = 1), the keys kept in the scratch arena.
 * FID_E_INVALID, nothing enqueued, outputs untouched: a NULL pointer, n <= 0, k < 1 or k > FID_TOPK_MAX, a NaN thresh, dim % 32 != 0.
 * Asynchronous on the context's stream; no host synchronisation beyond the scratch-arena rule of fid_match (see fid_gallery_group).
 * FID_TOPK_SLICES=<S> (read per call) forces the number of gallery slices the scan is cut into; the answer does not depend on it. */
#define FID_TOPK_MAX 32
int fid_gallery_search(fid_ctx *ctx, fid_gallery *g, const void *query_f16_dev, int n, int k, float thresh,
                       int32_t *idx_dev, float *score_dev);
/* Top-k over a gallery sharded by contiguous row blocks (the top-k twin of fid_match_keys / fid_match_merge below).  fid_topk_keys scans THIS
 * shard's rows (global index of its row 0 = first_row; first_row >= 0 and first_row + G_padded < 2^31) and writes keys_dev uint64 [n, k]: per
 * query its k best candidates as fid_match_keys' key, (order-preserving bits of the score << 32) | ~(first_row + row), descending, 0 = no
 * candidate.  Only scores > 0 that are not NaN become keys; no threshold yet.  After the shards' arrays have been all-gathered into
 * [parts, n, k], fid_topk_merge takes the k largest of a query's parts x k keys -- ignoring 0 and keys whose index is >= G_total -- and
 * applies the strict threshold: with contiguous shards exactly the answer of one fid_gallery_search over the whole gallery.
 * FID_E_INVALID as for fid_gallery_search, and parts <= 0, G_total <= 0, a first_row outside the range above. */
int fid_topk_keys(fid_ctx *ctx, fid_gallery *g, const void *query_f16_dev, int n, int k, int first_row,
                  uint64_t *keys_dev);
int fid_topk_merge(fid_ctx *ctx, const uint64_t *keys_dev, int parts, int n, int k, int G_total, float thresh,
                   int32_t *idx_dev, float *score_dev);
/* ---- Two-stage search: an exact int8 coarse scan for a shortlist, then the fp16 scores of the shortlist (opt-in; no default path uses it) ----
 * What vector stores ship as "quantised search with rescoring" (Qdrant, the store behind reference qdrant_manager.py, among them), with a
 * quantisation rule that is exact on every input, so the shortlist can be predicted to the bit.
 * The rule, for one unit fp16 row u[0 .. dim):  m = max |u_j|.  If m == 0 or any element is NaN or inf: e = 0 and every code 0 (the row scores 0
 * against everything and is never a candidate -- the rule of zero / deleted rows and NaN everywhere else).  Otherwise e = the smallest integer
 * with m <= 127 * 2^e and code_j = rint(u_j * 2^-e), ties to even, an int8 in [-127, 127]; u_j * 2^-e is exact in fp32, so each element is
 * rounded once.  Coarse score of (query q, row g) = ldexpf((float)dot_i32(code_q, code_g), e_q + e_g), exact for dim <= 1024
 * (|dot| <= 1024 * 127 * 127 < 2^24).  The coarse path needs dim % 64 == 0 and dim <= 1024, else FID_E_INVALID.
 * fid_quantize_rows_i8: n rows unit fp16 [n, dim] (8-byte aligned) -> codes int8 [n, dim], exps int8 [n]; asynchronous.  _host: the same on host arrays.
 * fid_gallery_quantize: gives the gallery an int8 copy of its rows (int8 [G_padded, dim] codes + int8 [G_padded] exponents, device memory owned
 * by the gallery, freed by fid_gallery_destroy); calling it again refreshes the copy.  fid_gallery_set_rows requantises exactly the rows it wrote,
 * when the copy exists; a gallery that never asked for it allocates and behaves as before.  Calls that write gallery rows on the device
 * (fid_gallery_group's NEW rows, fid_gallery_dedup's cleared rows) do NOT refresh it: call fid_gallery_quantize again after them.
 * fid_gallery_quant_data: a read-only view of the copy (FID_E_STATE without one). */
int fid_quantize_rows_i8(fid_ctx *ctx, const void *unit_f16_dev, int n, int dim, int8_t *codes_dev, int8_t *exps_dev);
int fid_quantize_rows_i8_host(const uint16_t *unit_f16, int n, int dim, int8_t *codes, int8_t *exps);
int fid_gallery_quantize(fid_ctx *ctx, fid_gallery *g);
int fid_gallery_quant_data(fid_gallery *g, const int8_t **codes_dev, const int8_t **exps_dev);
/* fid_coarse_keys: the int8 twin of fid_topk_keys.  Quantises the n queries (scratch arena), scans the gallery's int8 copy and writes keys_dev
 * uint64 [n, R], 1 <= R <= FID_TOPK_MAX: per query the R best rows by COARSE score in fid_topk_keys' key format, (order-preserving bits of the
 * coarse fp32 score << 32) | ~(first_row + row), descending, 0 = no candidate.  Only dot > 0 makes a key.  FID_E_STATE without a quantised copy.
 * FID_TOPK_SLICES forces the slice count here too; the answer does not depend on it.
 * fid_rerank_keys: for every non-zero key of keys_in_dev [n, R] that names a row of THIS gallery (first_row <= index < first_row + G; any other
 * key becomes 0) the score of (query, row) is recomputed from the fp16 rows -- fp32 accumulation in a fixed order, no atomics -- and the key is
 * rebuilt with it (0 if the score is <= 0 or NaN); keys_out_dev [n, R] (not keys_in_dev) receives each query's keys in descending order.  Its
 * output feeds fid_topk_merge unchanged: a row-sharded gallery runs fid_coarse_keys + fid_rerank_keys on the shard that owns the rows and merges
 * the all-gathered [parts, n, R] keys with fid_topk_merge(k = R), exactly as fid_topk_keys' output (the first k columns are the best k).  The shortlist is PER SHARD: a sharded search
 * keeps up to parts * R candidates per query and so may find more of the exact top k than the unsharded one, never fewer.
 * fid_gallery_search_coarse: fid_coarse_keys(first_row = 0), fid_rerank_keys, fid_topk_merge(parts = 1, k), keys in the scratch arena; needs
 * 1 <= k <= R <= FID_TOPK_MAX.  The output contract of fid_gallery_search: all n x k entries written, strict > max(0, thresh) on the RERANKED
 * score, (-1, 0.0) behind the last hit; FID_E_INVALID (a NULL pointer, n <= 0, k or R out of range, a NaN thresh, a dim the coarse path does not
 * take) enqueues nothing and leaves the outputs untouched.  Asynchronous on the context's stream.
 * NOT promised: a row whose exact score is among the k best but whose coarse score is not among the R best is missed.  Everything that IS reported
 * carries its exact fp16 score (fp32 sums in rerank order: equal to fid_gallery_search's wherever the sums are exact, within summation-order
 * rounding elsewhere), in the order and under the tie rule of fid_gallery_search. */
int fid_coarse_keys(fid_ctx *ctx, fid_gallery *g, const void *query_f16_dev, int n, int R, int first_row, uint64_t *keys_dev);
int fid_rerank_keys(fid_ctx *ctx, fid_gallery *g, const void *query_f16_dev, int n, int R, int first_row, const uint64_t *keys_in_dev,
                    uint64_t *keys_out_dev);
int fid_gallery_search_coarse(fid_ctx *ctx, fid_gallery *g, const void *query_f16_dev, int n, int k, int R, float thresh, int32_t *idx_dev,
                              float *score_dev);
/* Range search / similarity join: every (query, gallery row) with cosine >= thresh (and > 0), not the best k -- what the product layer's
 * duplicate merge asks of its vector store (reference smart_face_recognition.py:2761-2766: `search_similar(k=len(persons), threshold)`;
 * qdrant_manager.py:137-183, whose score_threshold keeps scores >= the threshold).  A zero (deleted / free) row and a NaN never hit.
 * query_f16_dev: unit fp16 [n, dim], or NULL = self-join (n is ignored; pairs i < j of the gallery's own rows, each once).
 * pairs_dev int32 [hit_cap, 2] = (query, row); scores_dev float [hit_cap]; total_dev uint64 [1] = number of hits found,
 * NOT clipped to hit_cap (total > hit_cap: hit_cap valid records, which ones is unspecified; call again with more room).
 * Record order is unspecified; the set and the scores are deterministic.  Asynchronous; no host synchronisation. */
int fid_gallery_range(fid_ctx *ctx, fid_gallery *g, const void *query_f16_dev, int n, float thresh,
                      int32_t *pairs_dev, float *scores_dev, long long hit_cap, uint64_t *total_dev);
/* Grouping a batch of visits into persons, in visit order: the reference's process_visit_data loop (smart_face_recognition.py:1721-2005, per-visit
 * body :1769-1951; the JSON twin :2077-2240 differs only in the threshold key) as ONE asynchronous call.  Per visit the reference runs
 * is_duplicate_image (:2618-2652: k = 1 search at duplicate_similarity_threshold = dup_thresh; a hit skips the visit), search_person (:1619-1643:
 * k = 5 at similarity_threshold = search_thresh), groups with the best hit when its similarity >= grouping_threshold_file / _json = group_thresh
 * (:1859-1861) and otherwise add_person (:1531-1602), which stores the embedding (qdrant_manager.py:91-136).  Its serial order (max_workers = 1)
 * is the one computed here.
 * query_f16_dev: n unit fp16 rows in visit order, as fid_l2_normalize_f16* writes them (16-byte aligned).  new_rows_dev: int32 [n_new_rows] gallery
 * rows the caller guarantees to be free (all zero) and distinct; the k-th NEW visit of the call is stored in new_rows[k].
 * Visit i is decided against the store AS VISIT i SEES IT: every gallery row as it was at the call plus the rows written for NEW visits < i.
 * best(i) = the maximum cosine over that store, lowest row among equal scores; a score that is not > 0 is no hit (score 0, row -1: the rule
 * of fid_match / fid_gallery_topk).  Verdicts, checked in this order:
 *   FID_VISIT_NO_FACE    the query row has no non-zero element (the all +0.0 row of a degenerate embedding, the -0.0-first marker row of an
 *                        empty slot).  Nothing stored, row -1, score 0, never anybody's candidate -- also behind a DEFERRED visit.
 *   FID_VISIT_DEFERRED   an earlier visit of this call needed a row when none of the n_new_rows was left: that visit and every (non-zero)
 *                        visit after it are NOT decided and not stored (row -1, score 0).  The decided prefix is exactly what a call on
 *                        that prefix alone returns; make room and call again with the suffix.
 *   FID_VISIT_DUPLICATE  best.score >= dup_thresh (:2636-2645; Qdrant's score_threshold keeps >=).  Nothing stored; row, score = best.
 *   FID_VISIT_RECOGNISED best.score >= search_thresh && best.score >= group_thresh (:1854-1861).  Nothing stored; row, score = best.
 *   FID_VISIT_NEW        otherwise: the query's fp16 row is copied BIT FOR BIT into gallery row new_rows[k], k = number of NEW verdicts
 *                        before it; row = that row; score = best.score if >= search_thresh else 0 (the `similarity` of :1855).
 * Outputs (device): verdict int32 [n], row int32 [n], score float [n], summary int32 [2] = {number of NEW, index of the first DEFERRED visit
 * or n}.  No gallery row outside new_rows[0 : summary[0]] is written.  An entry of new_rows outside [0, G) cannot be checked without a
 * synchronise: the visit is still NEW and consumes the entry, but NOTHING is stored, its row reads -1 and it is nobody's candidate.
 * Not here: the reference's "store is empty -> similarity 1.0" (:1820-1851; changes no decision -- engine.VectorGallery.group_visits reports
 * it), the SQL URL checks and add_person's md5 face_hash (an identical embedding scores 1.0 and is a DUPLICATE already).
 * FID_E_INVALID, nothing enqueued: a NULL pointer, n <= 0 or n > FID_GROUP_MAX_VISITS, n_new_rows < 0, a threshold that is NaN or <= 0
 * (the "> 0" hit rule makes it meaningless), dim % 32 != 0.  Asynchronous on the context's stream.  It does not synchronise with the host,
 * with the exception every entry point that uses a scratch arena shares (fid_match among them): the arena (1.3 MB here, sized for
 * FID_GROUP_MAX_VISITS at the first call, shared with fid_match) is replaced behind a stream synchronise when a call needs a larger one. */
enum { FID_VISIT_NEW = 0, FID_VISIT_RECOGNISED = 1, FID_VISIT_DUPLICATE = 2, FID_VISIT_NO_FACE = 3, FID_VISIT_DEFERRED = 4 };
#define FID_GROUP_MAX_VISITS 65536
int fid_gallery_group(fid_ctx *ctx, fid_gallery *g, const void *query_f16_dev, int n, float dup_thresh, float group_thresh,
                      float search_thresh, const int32_t *new_rows_dev, int n_new_rows, int32_t *verdict_dev, int32_t *row_dev,
                      float *score_dev, int32_t *summary_dev);
/* Merging duplicate persons of the store: the reference's maintenance pass find_and_merge_duplicates (smart_face_recognition.py:2726-2797, loop
 * :2755-2792, with merge_duplicate_persons :2679-2724; config.json merge_duplicate_threshold = 0.8) as ONE asynchronous call that returns one
 * keeper per person, not one record per pair.
 * rows_dev: int32 [n], the gallery rows of the persons IN PROCESSING ORDER (ascending person id); the caller guarantees they are distinct.  A
 * position TAKES PART when its row is inside [0, G) and holds a non-zero element (the sign bit does not count); any other position gets
 * keeper -1, score 0, and for an entry outside [0, G) nothing is read or written.
 * The rule, over positions k = 0 .. n - 1:  keeper[k] = the LOWEST position j < k with keeper[j] == -1 and hit(j, k), or -1 if there is none
 * ("the first person still alive absorbs me", not "the best score"); hit = the rule of fid_gallery_range: the cosine of the two stored fp16
 * unit rows, accumulated in fp32, is >= thresh and > 0 -- a zero (free / deleted) row and a NaN never hit.  Exact for any dependency depth.
 * Outputs (device), by position: keeper_dev int32 [n]; score_dev float [n] = the cosine of position k with its keeper, 0 where keeper is -1;
 * summary_dev int32 [2] = {positions absorbed, positions that took part}.
 * apply != 0: after the last decision every absorbed row is set to all +0.0 (the state fid_gallery_set_rows leaves for a zero embedding); no
 * other gallery byte is written.  apply == 0: the gallery is not written at all.
 * The reference's merge list is the absorbed positions sorted by (keeper, -score, id): engine.merges_from_keepers.
 * FID_E_INVALID, nothing enqueued, outputs untouched: a NULL pointer, n <= 0 or n > FID_DEDUP_MAX_ROWS, thresh NaN or <= 0, dim % 32 != 0.
 * Asynchronous on the context's stream; no host synchronisation beyond the scratch-arena rule of fid_match (see fid_gallery_group).  Scratch:
 * 12 bytes per position (no copy of the rows, no n x n or n x G matrix, no pair list). */
#define FID_DEDUP_MAX_ROWS (1 << 20)
int fid_gallery_dedup(fid_ctx *ctx, fid_gallery *g, const int32_t *rows_dev, int n, float thresh, int apply,
                      int32_t *keeper_dev, float *score_dev, int32_t *summary_dev);
/* Density clusters of stored faces: "which of these n faces are the same person" as ONE asynchronous call whose answer does not depend on the
 * order of the rows (fid_gallery_group and fid_gallery_dedup replay the reference's greedy loops and do).  No reference analogue: its
 * `clustering_results/` are written by the greedy visit loop.
 * rows_dev: int32 [n], the gallery row of every position k = 0 .. n - 1, as in fid_gallery_dedup; NULL = positions are the gallery rows
 * 0 .. G - 1 and n is ignored.  A position TAKES PART when its row is inside [0, G) and holds a non-zero element (the sign bit does not count).
 * hit(j, k) = the rule of fid_gallery_range: the fp32 cosine of the two stored fp16 rows is >= thresh and > 0.  A NaN never hits; a position
 * that takes no part never hits and is never hit.
 *   degree[k] = 1 + the number of OTHER positions that take part and hit k; 0 for a position that takes no part.
 *   core[k]   = degree[k] >= min_pts (DBSCAN's min_samples: the point itself counts).
 *   cluster   = a connected component of the hit graph restricted to core positions; its label is the LOWEST core position in it
 *               (canonical: independent of any processing order).
 *   via[k]    = for a position that takes part, the core position c != k with hit(c, k) and the highest score, the lowest position among
 *               equal scores; score[k] = that cosine.  via -1 and score 0 when there is no such core.
 *   label[k]  = a core's: its cluster's label.  A non-core position with via >= 0 is a BORDER: the label of via[k].  This is a deterministic
 *               rule of this library -- sklearn's DBSCAN gives a border point to whichever cluster reaches it first.  Everything else: -1; a
 *               position that takes part and has label -1 is NOISE.
 * min_pts = 1 makes every position that takes part a core: plain connected components, singletons as clusters of one.
 * Outputs (device), by position: label_dev, degree_dev, via_dev int32 [n]; score_dev float [n]; summary_dev int32 [6] = {clusters, cores,
 * borders, noise, took part, fault}.  fault != 0: a union-find loop reached its bound of n + 1 steps, which no correct run does -- the labels
 * are not to be trusted (the Python layer raises).
 * FID_E_INVALID, nothing enqueued, outputs untouched: a NULL context, gallery or output pointer, n <= 0 or n > FID_CLUSTER_MAX_ROWS,
 * min_pts < 1, thresh NaN or <= 0, dim % 32 != 0, a gallery beyond what a buffer descriptor addresses (4 GiB, as fid_gallery_range).
 * Asynchronous on the context's stream; no host synchronisation beyond the scratch-arena rule of fid_match (see fid_gallery_group).  The
 * gallery is never written.  Scratch: 12 bytes per position and one bit per pair of 128-position tiles (4 MB at 2^20 positions): no n x n
 * matrix, no pair list.  FID_CLUSTER_SKIP=0 in the environment (read per call; measurements) makes the second pass compute every tile pair
 * again instead of only those the first pass found a hit in; the answer does not depend on it.
 * fid_cluster_host: the same rule in plain loops on HOST arrays (csrc/cluster_core.h), no device involved: rows_f16 [G, dim] fp16 rows in
 * place of the gallery (any dim >= 1), rows int32 [n] or NULL, outputs as above.  Its cosine is the fp32 sum in ascending column order; the
 * device sums in the order of its tiles.  Where the sums are exact the two are equal to the bit; elsewhere a pair within summation-order
 * rounding of the threshold may fall on either side. */
#define FID_CLUSTER_MAX_ROWS (1 << 20)
int fid_gallery_cluster(fid_ctx *ctx, fid_gallery *g, const int32_t *rows_dev, int n, float thresh, int min_pts, int32_t *label_dev,
                        int32_t *degree_dev, int32_t *via_dev, float *score_dev, int32_t *summary_dev);
int fid_cluster_host(const void *rows_f16, int G, int dim, const int32_t *rows, int n, float thresh, int min_pts, int32_t *label,
                     int32_t *degree, int32_t *via, float *score, int32_t *summary);
/* Genuine / impostor score distributions of LABELLED stored faces: what the thresholds of this library are calibrated with.  Over all pairs of
 * labelled faces, how are same-person and different-person cosines distributed, which threshold gives a wanted false-accept rate, and which
 * stored faces are probably mislabelled -- as ONE asynchronous call.  No reference analogue: its thresholds are constants of config.json.
 * rows_dev: int32 [n], the gallery row of every position k = 0 .. n - 1, exactly as in fid_gallery_cluster; NULL = positions are the gallery
 * rows 0 .. G - 1 and n is ignored.  labels_dev: int32 [n], the person of every position; a negative label = unlabelled.
 * A position TAKES PART when its row is inside [0, G), the row holds a non-zero element (the sign bit does not count) and its label is >= 0;
 * any other position is in no pair.
 * Every unordered pair i < j of positions that take part is counted once.  s = the fp32 cosine of the two stored fp16 rows, from the same tile
 * arithmetic and therefore the same sums as fid_gallery_cluster.  The pair is GENUINE when the two labels are equal, IMPOSTOR otherwise.
 *   bin:  a non-finite s goes into no bin and is counted in summary[3].  Otherwise b = (int)floorf(s * (float)(bins / 2)) + bins / 2, clamped
 *         to [0, bins - 1]: ONE rounded fp32 multiply.  bins is even, 2 .. FID_HIST_MAX_BINS.  With bins a power of two the multiply is exact:
 *         bin b holds exactly the scores with -1 + 2 b / bins <= s < -1 + 2 (b + 1) / bins, and s = 1 lands in the last bin.  So for a
 *         power-of-two bins the cumulative count from bin b upward is EXACTLY the number of pairs that `s >= thresh` accepts at
 *         thresh = -1 + 2 b / bins -- for a thresh > 0 that is the hit rule of fid_gallery_range / fid_gallery_cluster.  For any other even
 *         bins an edge is exact only up to the rounding of that one multiply.
 *   hardest pairs, per position (what finds label errors in an enrolment set):
 *         imp_via[k] = the position j != k of ANOTHER label with the HIGHEST finite score, gen_via[k] = the position j != k of the SAME label
 *         with the LOWEST finite score; among equal scores the lowest position.  imp_score[k] / gen_score[k] = that score.  -1 and 0.0f where
 *         there is no such pair or the position takes no part.  Scores are ordered by their order-preserving bit pattern (csrc/calib_core.h):
 *         the order of the numbers, with -0.0 BELOW +0.0.  Every sum starts from +0.0, so a -0.0 score does not arise; the rule only pins
 *         the corner (tests/calib_oracle.py orders the same way).
 * Outputs (device): hist_dev uint64 [2][bins], genuine first, then impostor; imp_via_dev, gen_via_dev int32 [n]; imp_score_dev, gen_score_dev
 * float [n]; summary_dev uint64 [4] = {positions that took part, genuine pairs, impostor pairs, non-finite pairs} (the pair totals are the
 * sums of the two histograms).  hist_dev and summary_dev must be 8-byte aligned.  Integer sums only: the answer is the same bytes on every run.
 * FID_E_INVALID, nothing enqueued, outputs untouched: a NULL context, gallery, labels or output pointer (or a misaligned one), n <= 0 or
 * n > FID_HIST_MAX_ROWS, bins odd or outside 2 .. FID_HIST_MAX_BINS, dim % 32 != 0, a gallery beyond what a buffer descriptor addresses
 * (4 GiB, as fid_gallery_cluster).
 * Asynchronous on the context's stream; no host synchronisation beyond the scratch-arena rule of fid_match (see fid_gallery_group).  The
 * gallery is never written.  Scratch: 16 bytes per position: no n x n matrix, no pair list.  FID_HIST_PEEL (0, the default, or 4: rounds of in-wave
 * aggregation before the LDS counters) and FID_HIST_GRID (workgroups of the pass) in the environment are read per call, for measurements;
 * the answer depends on neither.
 * fid_score_hist_host: the same rule in plain loops on HOST arrays (csrc/calib_core.h), no device involved: rows_f16 [G, dim] fp16 rows in
 * place of the gallery (any dim >= 1), rows int32 [n] or NULL, labels int32 [n], outputs as above.  Its cosine is the fp32 sum in ascending
 * column order starting from +0.0f; the device sums in the order of its tiles.  Where the sums are exact the two are equal to the bit;
 * elsewhere a score within summation-order rounding of a bin edge may fall on either side. */
#define FID_HIST_MAX_ROWS (1 << 20)
#define FID_HIST_MAX_BINS 4096
int fid_gallery_score_hist(fid_ctx *ctx, fid_gallery *g, const int32_t *rows_dev, const int32_t *labels_dev, int n, int bins,
                           uint64_t *hist_dev, int32_t *imp_via_dev, float *imp_score_dev, int32_t *gen_via_dev, float *gen_score_dev,
                           uint64_t *summary_dev);
int fid_score_hist_host(const void *rows_f16, int G, int dim, const int32_t *rows, const int32_t *labels, int n, int bins,
                        uint64_t *hist, int32_t *imp_via, float *imp_score, int32_t *gen_via, float *gen_score, uint64_t *summary);
/* Identity templates: ONE gallery row per person from MANY stored faces -- the weighted mean of the person's stored rows, re-normalised, with
 * the faces that disagree with the mean left out -- as ONE asynchronous call.  No reference analogue: its build_targets takes one photograph per
 * name.  The sums are taken EXACTLY, in integers, so the answer is the same bytes whatever the order of the positions, the launch geometry or
 * the arrival order of an atomic: device, host twin and tests/template_oracle.py agree byte for byte on ANY input.
 * Positions: rows_dev int32 [n], the gallery row of every position k = 0 .. n - 1, exactly as in fid_gallery_cluster / fid_gallery_score_hist;
 * NULL = positions are the gallery rows 0 .. G - 1 and n is ignored.  A row may occur at several positions.  labels_dev int32 [n]: the person
 * of position k.  weights_dev int32 [n]: an integer weight; NULL = every weight is 1.
 * A position TAKES PART (is a MEMBER of person labels[k]) when its row is inside [0, G), 0 <= label < P, 1 <= weight <= 255, the row holds a
 * non-zero element (the sign bit does not count) and every element of the row is finite with |x| <= 2 (stored rows are unit rows: the element
 * condition only pins corners).  A position whose row, label and weight are in range but whose elements fail is counted in summary[4].  No
 * other position takes part in any sum.
 *   sum:      an fp16 number with |x| <= 2 is an integer multiple of 2^-24: X_kc = x_kc * 2^24 is an exact integer with |X| <= 2^25.
 *             S_pc = sum of w_k * X_kc over the members of p, in int64.  With n <= FID_TEMPLATE_MAX_ROWS = 2^20 and w <= 255:
 *             |S| <= 2^20 * 255 * 2^25 < 2^53, so the sum cannot overflow and its conversion to double is exact.
 *   norm:     the only floating-point reduction of the call, so its order is part of the ABI.  q_c = (double)S_c * (double)S_c, rounded.
 *             Lane l of 64 owns the columns c with (c / 8) % 64 == l -- eight consecutive columns of every block of 512, what a 16-byte load
 *             per lane brings -- and adds its q_c in ascending c, starting from +0.0 (columns at or beyond dim contribute nothing).  Six
 *             butterfly rounds follow, lane l adding lane l ^ o for o = 32, 16, 8, 4, 2, 1, then sqrt.  Every operation is a separately
 *             rounded IEEE fp64 operation, no FMA contraction.  (numpy: q padded to a multiple of 512, reshape(-1, 64, 8), a sequential add
 *             over the first and then the last axis index, six folds.)
 *   template: t_c = (double)S_c / nrm in fp64, rounded to fp32, then rounded to fp16, both to nearest even (numpy:
 *             .astype(float32).astype(float16)).  If S is the zero vector (no member, or members that cancel) the template is the all-zero
 *             row, which every search of this library treats as empty.
 *   trimming: one round.  T_c = the fp16 template as an integer, as above; D_k = sum over c of X_kc * T_c in int64 (|D| <= 2^49 * dim);
 *             score[k] = (float)((double)D_k * 2^-48), each conversion rounded to nearest once.  A member is KEPT when score[k] >= min_score,
 *             compared in fp32; min_score <= -2 keeps every member (the scores are still reported).  The final template of a person is the
 *             rule above on its kept members only; with nothing dropped it is the first one.  A person whose members are all dropped gets
 *             the zero row.  The reported score is the one the decision used: against the FIRST template.
 * Outputs (device): templates_f16_dev fp16 [P, dim] (16-byte aligned); score_dev float [n] (0.0f for a position that takes no part); kept_dev
 * int32 [n]: 1 kept, 0 dropped, -1 takes no part; person_dev int32 [P, 4] = {members, kept members, position of the lowest-scoring member,
 * position of the highest-scoring member} (the lowest position among equal scores; -1 where there is no member); cohesion_dev float [P] =
 * (float)(nrm_final / ((double)W_kept * 16777216.0)), W_kept the weights of the kept members: the resultant length of the weighted mean,
 * in [0, 1] for unit rows, 1 when all kept faces are the same vector, 0.0f for a zero template; summary_dev int64 [6] (8-byte aligned) =
 * {positions that took part, persons with >= 1 member, persons (of all P) with a zero template, positions dropped, positions rejected for their
 * elements, 0}.
 * FID_E_INVALID, nothing enqueued, outputs untouched: a NULL context, gallery, labels or output pointer, a misaligned summary_dev or
 * templates_f16_dev, n <= 0 or n > FID_TEMPLATE_MAX_ROWS, P <= 0 or P > n, a non-finite min_score, dim % 32 != 0 or
 * dim > FID_TEMPLATE_MAX_DIM, a gallery beyond 4 GiB (as fid_gallery_score_hist).
 * Asynchronous on the context's stream; no host synchronisation beyond the scratch-arena rule of fid_match (see fid_gallery_group).  The
 * gallery is never written.  Scratch: 12 bytes per position, 48 per person, and one accumulator row of int64 per person with more than
 * FID_TEMPLATE_CHUNK members (room for n / (FID_TEMPLATE_CHUNK + 1) rows): no [P, dim] array of sums.  A wave sums up to FID_TEMPLATE_CHUNK
 * members; a person with more is split, and its chunks combine through 64-bit integer atomic adds.  FID_TEMPLATE_CHUNK (16 .. 65536) in the
 * environment overrides the chunk per call, and FID_TEMPLATE_COMBINE=pass replaces the atomics by partial rows (one per chunk of a split person, at
 * most 2 n / chunk + 1) and a second pass that adds them up, both for measurements; the answer depends on neither.
 * fid_templates_host: the same rule in plain loops on HOST arrays (csrc/template_core.h), no device involved: rows_f16 [G, dim] fp16 rows in
 * place of the gallery (any dim 1 .. FID_TEMPLATE_MAX_DIM), rows / weights int32 [n] or NULL, outputs as above, equal to the device's byte
 * for byte.
 * fid_gallery_put_rows_f16: gallery row rows_dev[i] = the fp16 row i of src_f16_dev [n, dim] (device memory, 16-byte aligned), byte for byte:
 * no re-normalisation, where fid_gallery_set_rows takes host fp32 and rounds again.  How templates enter a gallery where they lie.  The rows
 * are checked on the host first (one small download, so the call waits for the work enqueued before it): a row outside [0, G) refuses the
 * whole call with FID_E_INVALID and nothing is written.  Rows should be distinct (which source wins otherwise is unspecified).  Like
 * fid_gallery_group it does not refresh the int8 copy of fid_gallery_quantize: quantise again before the next coarse search. */
#define FID_TEMPLATE_MAX_ROWS (1 << 20)
#define FID_TEMPLATE_MAX_DIM 4096
#define FID_TEMPLATE_CHUNK 256
int fid_gallery_templates(fid_ctx *ctx, fid_gallery *g, const int32_t *rows_dev, const int32_t *labels_dev, const int32_t *weights_dev, int n,
                          int P, float min_score, void *templates_f16_dev, float *score_dev, int32_t *kept_dev, int32_t *person_dev,
                          float *cohesion_dev, int64_t *summary_dev);
int fid_templates_host(const void *rows_f16, int G, int dim, const int32_t *rows, const int32_t *labels, const int32_t *weights, int n, int P,
                       float min_score, void *templates_f16, float *score, int32_t *kept, int32_t *person, float *cohesion, int64_t *summary);
int fid_gallery_put_rows_f16(fid_ctx *ctx, fid_gallery *g, const int32_t *rows_dev, const void *src_f16_dev, int n);
/* Gallery sharded over ranks by contiguous row blocks (the 1 M-entry variant of main.py:136-142):
 * fid_match_keys scans THIS rank's rows (global index of its row 0 = first_row) for all n queries and writes one
 * packed key per query, (order-preserving bits of the score << 32) | ~global_index; after the ranks' key arrays
 * have been all-gathered ([parts, n], 8 bytes per query and rank) fid_match_merge takes the maximum key per query
 * = the best score, lowest global index on ties, and applies the strict '>' threshold like fid_match. */
int fid_match_keys(fid_ctx *ctx, fid_gallery *g, const void *query_f16_dev, int n, int first_row,
                   uint64_t *keys_dev);
int fid_match_merge(fid_ctx *ctx, const uint64_t *keys_dev, int parts, int n, int G_total, float thresh,
                    int32_t *idx_dev, float *score_dev);

/* ---- 1:1 verification: P pairs of embeddings -> P (score, verdict) records and the counters of the batch loop.  Replaces the reference's
 * compare_face_images (smart_face_recognition.py:878-963), calculate_face_similarity (:965-982) and the tallies of process_face_comparisons
 * (:1088-1094, :1108-1110); compare_face_from_api.py is the same workflow as a script.
 * emb_dev [n_rows, dim]: RAW fp32 embeddings, e.g. the recogniser's output tensor (fid_net_tensor) as it is -- not normalised, not fp16.
 * pairs_dev int32 [P, 2] names the two sides of each pair:
 *   offsets_dev == NULL: entries are rows of emb_dev; -1 = the image is missing (FID_PAIR_NO_IMAGE); -2 or any other value outside
 *                        [0, n_rows) = no face (FID_PAIR_NO_FACE).
 *   offsets_dev int32 [n_img + 1] (what fid_face_pack writes with max_per_frame = 1): entries are image indices; -1 or any value outside
 *                        [0, n_img) = FID_PAIR_NO_IMAGE; image i is row offsets[i] when offsets[i+1] > offsets[i] and 0 <= offsets[i] < n_rows,
 *                        otherwise FID_PAIR_NO_FACE.
 *   NO_IMAGE on either side wins over NO_FACE (the reference checks the downloads first, :896, then the faces, :915).  A row that is not
 *   valid is never read.
 * labels_dev (optional, may be NULL) int32 [P]: 1 / 0 = the API's `approve` of the pair, any other value (-1) = none.
 * Outputs (device): score float [P], verdict int32 [P] (FID_PAIR_*).  A valid pair: three fp32 sums a.b, a.a, b.b reduced in a fixed order
 * (bitwise reproducible), score = dot / (sqrtf(aa) * sqrtf(bb)) in the reference's order (:978) with correctly rounded divide and square root;
 * FID_PAIR_SAME iff score > thresh, strictly (:932).  A zero row gives a NaN score and FID_PAIR_DIFFERENT, as `nan > t` does in the reference.
 * An error pair: score = 0.0f (the reference's 'confidence': 0.0).
 * counters_dev int32 [8] is ADDED TO, never cleared (zero it once with fid_memset; chunks then sum up): 0 processed, 1 same, 2 different,
 * 3 no-image errors, 4 no-face errors, 5 labelled pairs, 6 labelled pairs whose label == (verdict == FID_PAIR_SAME) -- an error pair counts as
 * "not same" (:1082) --, 7 untouched.
 * FID_E_INVALID, nothing enqueued, outputs untouched: P < 0, n_rows < 0, n_img < 0, dim <= 0 or dim % 4 != 0, emb_dev not 16-byte aligned,
 * emb_dev == NULL with n_rows > 0, a NULL pair table or output pointer with P > 0.  P == 0 returns FID_OK without a launch.
 * One launch, asynchronous on the context's stream, no scratch arena. */
#define FID_PAIR_DIFFERENT 0
#define FID_PAIR_SAME      1
#define FID_PAIR_NO_IMAGE  2   /* 'Could not download one or both images' (:896-903) */
#define FID_PAIR_NO_FACE   3   /* 'Could not detect faces in one or both images' (:915-922) */
int fid_pair_verify(fid_ctx *ctx, const float *emb_dev, int n_rows, int dim, const int32_t *pairs_dev, int P,
                    const int32_t *offsets_dev, int n_img, const int32_t *labels_dev, float thresh, float *score_dev,
                    int32_t *verdict_dev, int32_t *counters_dev);

/* ---- the path's one collective (no reference analogue: the reference is single-process; spec = BASELINE.json
 * north_star "a single RCCL all-gather over xGMI of per-rank embeddings before the gallery match").
 * One process per GPU.  Rank 0 calls fid_comm_unique_id and the host hands the FID_COMM_ID_BYTES bytes to every
 * rank (file, environment, MPI, a torch.distributed store ...); every rank then calls fid_comm_init_rank (collective,
 * blocks until all ranks arrived).  fid_allgather enqueues ncclAllGather on the context's stream:
 * recv_dev [nranks][bytes_per_rank] <- each rank's send_dev, in rank order. */
#define FID_COMM_ID_BYTES 128
int fid_comm_unique_id(void *id_out, size_t bytes);
int fid_comm_init_rank(fid_ctx *ctx, int nranks, int rank, const void *id, size_t bytes, fid_comm **out);
int fid_comm_destroy(fid_ctx *ctx, fid_comm *comm);
int fid_comm_info(fid_comm *comm, int *nranks, int *rank);
int fid_allgather(fid_ctx *ctx, fid_comm *comm, const void *send_dev, void *recv_dev, size_t bytes_per_rank);

/* full cosine matrix fp32 [n, G_padded] (row stride = G_padded, a multiple of 32; columns >= G are
 * 0): tests / compute_similarity parity.  Caller-allocated device memory. */
int fid_cosine_matrix(fid_ctx *ctx, fid_gallery *g, const void *query_f16_dev, int n,
                      float *out_dev);

#ifdef __cplusplus
}
#endif
#endif /* FACEID_H */
