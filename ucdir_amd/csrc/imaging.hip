// libucdir_hip: the val loop's imaging operators (include/ucdir_hip.h): PSNR / SSIM, the JPEG round trip, encoder and decoder,
// the Pillow resampler, NIQE and the real-world SR degradations.  Stateless entries: each runs on the device its first
// buffer lives on.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "../../include/ucdir_hip.h"
#include "api_common.h"
#include "image_metrics.hip.h"
#include "jpeg_roundtrip.hip.h"
#include "jpeg_encode.hip.h"
#include "jpeg_decode.hip.h"
#include "resample.hip.h"
#include "niqe.hip.h"
#include "realsr.hip.h"

extern "C" {

// val-loop scores (csrc/image_metrics.hip.h): tiles of IM_TW x IM_TR valid-region outputs; at least one tile per (image, channel)
// so that the SSE of images below 11 x 11 is still counted
static void image_metrics_grid(int32_t H, int32_t W, int& nx, int& ny) {
    const int hg = H > 10 ? H - 10 : 1, wg = W > 10 ? W - 10 : 1;
    nx = (wg + IM_TW - 1) / IM_TW;
    ny = (hg + IM_TR - 1) / IM_TR;
}

int64_t ucdir_image_metrics_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return -1;
    int nx, ny;
    image_metrics_grid(H, W, nx, ny);
    return (int64_t)B * C * nx * ny * (int64_t)(sizeof(double) + sizeof(unsigned long long));
}

int32_t ucdir_image_metrics(const float* a, int64_t a_sn, int64_t a_sc, int64_t a_sh, const float* b, int64_t b_sn, int64_t b_sc,
                            int64_t b_sh, int32_t B, int32_t C, int32_t H, int32_t W, void* workspace, uint64_t* sse, double* ssim_sum,
                            void* stream) {
    API_BEGIN
    const std::string w("ucdir_image_metrics");
    require(a && b && workspace && sse && ssim_sum, w + ": null argument");
    require(B > 0 && H > 0 && W > 0, w + ": bad shape");
    require(C == 1 || C == 3, w + ": C must be 1 or 3");
    require((int64_t)B * C <= 65535, w + ": more than 65535 (image, channel) pairs");
    require(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)sse & 7) == 0 && ((uintptr_t)ssim_sum & 7) == 0,
            w + ": workspace and outputs must be 8-byte aligned");
    const void* others[4] = {b, workspace, sse, ssim_sum};
    const char* names[4] = {"b", "workspace", "sse", "ssim_sum"};
    const int device = same_device(w, a, "a", others, names, 4);
    int nx, ny;
    image_metrics_grid(H, W, nx, ny);
    const long long ntiles = (long long)nx * ny;
    require(ntiles <= 0x7fffffffLL, w + ": image too large");
    // the 11-tap Gaussian of metrics._ssim, normalised with numpy's summation order for 11 float64 values
    ImageMetricsTaps taps;
    for (int k = 0; k < 11; ++k) taps.w[k] = std::exp(-(double)((k - 5) * (k - 5)) / (2 * 1.5 * 1.5));
    double tot = ((taps.w[0] + taps.w[1]) + (taps.w[2] + taps.w[3])) + ((taps.w[4] + taps.w[5]) + (taps.w[6] + taps.w[7]));
    tot += taps.w[8];
    tot += taps.w[9];
    tot += taps.w[10];
    for (int k = 0; k < 11; ++k) taps.w[k] /= tot;
    DevGuard dg(device);
    double* part_ssim = (double*)workspace;
    unsigned long long* part_sse = (unsigned long long*)(part_ssim + (long long)B * C * ntiles);
    hipLaunchKernelGGL(image_metrics_tile_kernel, dim3((unsigned)ntiles, (unsigned)(B * C)), dim3(256), 0, (hipStream_t)stream,
                       a, (long long)a_sn, (long long)a_sc, (long long)a_sh, b, (long long)b_sn, (long long)b_sc, (long long)b_sh,
                       C, H, W, nx, ny, taps, part_ssim, part_sse);
    HIPC(hipGetLastError());
    hipLaunchKernelGGL(image_metrics_finish_kernel, dim3((unsigned)(B * C)), dim3(256), 0, (hipStream_t)stream, part_ssim, part_sse,
                       (int)ntiles, (int)(H > 10 && W > 10), (unsigned long long*)sse, ssim_sum);
    HIPC(hipGetLastError());
    API_END
}

// Annex K luma table and the top-left 4 x 4 of the chroma table (99 everywhere else), natural order: the JPEG codecs and DiffJPEG
static const int std_luma[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                                 14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                                 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
static const int std_chroma4[16] = {17, 18, 24, 47, 18, 21, 26, 66, 24, 26, 56, 99, 47, 66, 99, 99};

// Annex K quantisation tables with IJG quality scaling (jcparam.c jpeg_quality_scaling + jpeg_add_quant_table, force_baseline),
// natural order
static void jpeg_quant_tables(int quality, int (*q)[64]) {
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int i = 0; i < 64; ++i) {
        const int r = i >> 3, c = i & 7;
        const int sc = (r < 4 && c < 4) ? std_chroma4[r * 4 + c] : 99;
        q[0][i] = std::min(std::max((std_luma[i] * scale + 50) / 100, 1), 255);
        q[1][i] = std::min(std::max((sc * scale + 50) / 100, 1), 255);
    }
}

// JPEG round trip of the JPEG-restoration val task (csrc/jpeg_roundtrip.hip.h): the Y plane of the 16-padded image and two half-size
// chroma planes per image
int64_t ucdir_jpeg_roundtrip_workspace_bytes(int32_t B, int32_t H, int32_t W) {
    if (B <= 0 || H < 16 || W < 16) return -1;
    const int64_t H16 = (H + 15) & ~15, W16 = (W + 15) & ~15;
    return (int64_t)B * H16 * W16 * 3 / 2;
}

int32_t ucdir_jpeg_roundtrip(const uint8_t* in, uint8_t* out, int32_t B, int32_t H, int32_t W, int32_t quality, int32_t bgr,
                             void* workspace, void* stream) {
    API_BEGIN
    const std::string w("ucdir_jpeg_roundtrip");
    require(quality >= 1 && quality <= 100, w + ": quality must lie in 1..100");
    require(B > 0 && H >= 16 && W >= 16, w + ": bad shape (B > 0, H and W at least 16)");
    require((int64_t)B * H * W < (1LL << 31), w + ": more than 2^31 - 1 pixels");
    require(in && out && workspace, w + ": null argument");
    require(((uintptr_t)workspace & 7) == 0, w + ": workspace must be 8-byte aligned");
    const void* others[2] = {out, workspace};
    const char* names[2] = {"out", "workspace"};
    const int device = same_device(w, in, "in", others, names, 2);
    JpegQuant qt;
    jpeg_quant_tables(quality, qt.q);
    DevGuard dg(device);
    const long long nmcu = (long long)B * ((H + 15) / 16) * ((W + 15) / 16);
    hipLaunchKernelGGL(jpeg_mcu_kernel, dim3((unsigned)((nmcu + JPEG_MCUS_PER_WG - 1) / JPEG_MCUS_PER_WG)), dim3(256), 0,
                       (hipStream_t)stream, in, (unsigned char*)workspace, B, H, W, bgr ? 1 : 0, qt);
    HIPC(hipGetLastError());
    const long long npix = (long long)B * H * W;
    hipLaunchKernelGGL(jpeg_upsample_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned char*)workspace, out, B, H, W, bgr ? 1 : 0);
    HIPC(hipGetLastError());
    API_END
}

// Baseline JPEG encoder of the val loop's files (csrc/jpeg_encode.hip.h).  Workspace, every part 16-byte aligned: the
// zigzag coefficients, per-block and per-group bit offsets, per-image bit totals, per-chunk 0xFF counts, the unstuffed bitstream.
struct JpegEncLayout {
    int64_t nblk, ngrp, rawcap, nchunk;                   // blocks and groups per image, stream words and chunks per image
    int64_t coef, boff, part, totbits, ffpart, raw, bytes;
};

static const char* jpeg_encode_check(int32_t B, int32_t H, int32_t W, int32_t sub) {
    if (sub != 0 && sub != 2) return "unknown subsampling (0: 4:4:4, 2: 4:2:0)";
    if (B < 1 || H < 1 || W < 1) return "bad shape (B, H and W at least 1)";
    if (B > 65535) return "more than 65535 images";
    if (H > 65535 || W > 65535) return "sides above 65535 do not fit a JPEG frame header";
    if (jpeg_enc::blocks_per_image(H, W, sub) > jpeg_enc::MAX_BLOCKS) return "more than 2^21 blocks per image (32-bit bit offsets)";
    return nullptr;
}

static JpegEncLayout jpeg_encode_layout(int32_t B, int32_t H, int32_t W, int32_t sub) {
    JpegEncLayout l;
    auto up16 = [](int64_t v) { return (v + 15) / 16 * 16; };
    l.nblk = jpeg_enc::blocks_per_image(H, W, sub);
    l.ngrp = (l.nblk + JPEG_ENC_GROUP - 1) / JPEG_ENC_GROUP;
    l.rawcap = jpeg_enc::raw_cap_words(l.nblk);
    l.nchunk = (l.rawcap * 4 + JPEG_ENC_CHUNK - 1) / JPEG_ENC_CHUNK;
    l.coef = 0;
    l.boff = l.coef + up16((int64_t)B * l.nblk * 128);
    l.part = l.boff + up16((int64_t)B * l.nblk * 4);
    l.totbits = l.part + up16((int64_t)B * l.ngrp * 4);
    l.ffpart = l.totbits + up16((int64_t)B * 4);
    l.raw = l.ffpart + up16((int64_t)B * l.nchunk * 4);
    l.bytes = l.raw + (int64_t)B * l.rawcap * 4;
    return l;
}

int64_t ucdir_jpeg_encode_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t subsampling) {
    if (jpeg_encode_check(B, H, W, subsampling)) return -1;
    return jpeg_encode_layout(B, H, W, subsampling).bytes;
}

int64_t ucdir_jpeg_encode_bound(int32_t H, int32_t W, int32_t subsampling) {
    if (jpeg_encode_check(1, H, W, subsampling)) return -1;
    const int64_t stream = (jpeg_enc::blocks_per_image(H, W, subsampling) * jpeg_enc::MAX_BLOCK_BITS + 7) / 8;
    return jpeg_enc::HEADER_BYTES + 2 * stream + 2;
}

int32_t ucdir_jpeg_encode_header(int32_t H, int32_t W, int32_t quality, int32_t subsampling, uint8_t* out, int32_t cap) {
    try {
        const std::string w("ucdir_jpeg_encode_header");
        require(quality >= 1 && quality <= 100, w + ": quality must lie in 1..100");
        const char* bad = jpeg_encode_check(1, H, W, subsampling);
        require(!bad, w + ": " + (bad ? bad : ""));
        require(out, w + ": null argument");
        require(cap >= jpeg_enc::HEADER_BYTES, w + ": cap is below the 623 bytes of the header");
        int q[2][64];
        jpeg_quant_tables(quality, q);
        return jpeg_enc::write_header(H, W, subsampling, q, out);
    } catch (const std::exception& e) {
        g_err = e.what();
        return -1;
    }
}

int32_t ucdir_jpeg_encode(const uint8_t* in, uint8_t* out, int32_t* lengths, int32_t B, int32_t H, int32_t W, int32_t quality,
                          int32_t subsampling, int32_t bgr, void* workspace, void* stream) {
    API_BEGIN
    const std::string w("ucdir_jpeg_encode");
    require(quality >= 1 && quality <= 100, w + ": quality must lie in 1..100");
    const char* bad = jpeg_encode_check(B, H, W, subsampling);
    require(!bad, w + ": " + (bad ? bad : ""));
    require((int64_t)B * H * W < (1LL << 31), w + ": more than 2^31 - 1 pixels");
    require(in && out && lengths && workspace, w + ": null argument");
    require(((uintptr_t)workspace & 15) == 0, w + ": workspace must be 16-byte aligned");
    require(((uintptr_t)lengths & 3) == 0, w + ": lengths must be 4-byte aligned");
    const void* others[3] = {out, lengths, workspace};
    const char* names[3] = {"out", "lengths", "workspace"};
    const int device = same_device(w, in, "in", others, names, 3);
    const JpegEncLayout l = jpeg_encode_layout(B, H, W, subsampling);
    const long long stride = ucdir_jpeg_encode_bound(H, W, subsampling);
    JpegQuant qt;
    jpeg_quant_tables(quality, qt.q);
    JpegEncHeader header;                                  // a kernel argument of the scatter kernel: no copy, nothing to outlive
    unsigned char hdr[sizeof(header.w)] = {0};
    require(jpeg_enc::write_header(H, W, subsampling, qt.q, hdr) == jpeg_enc::HEADER_BYTES, w + ": header size");
    std::memcpy(header.w, hdr, sizeof(hdr));
    DevGuard dg(device);
    hipStream_t st = (hipStream_t)stream;
    unsigned char* ws = (unsigned char*)workspace;
    short* coef = (short*)(ws + l.coef);
    unsigned int* boff = (unsigned int*)(ws + l.boff);
    unsigned int* part = (unsigned int*)(ws + l.part);
    unsigned int* totbits = (unsigned int*)(ws + l.totbits);
    unsigned int* ffpart = (unsigned int*)(ws + l.ffpart);
    unsigned int* raw = (unsigned int*)(ws + l.raw);
    HIPC(hipMemsetAsync(raw, 0, (size_t)B * l.rawcap * 4, st));
    const long long units = (l.nblk + 5) / 6;
    const dim3 gblocks((unsigned)((units + 3) / 4), (unsigned)B), ggrp((unsigned)l.ngrp, (unsigned)B), gchunk((unsigned)l.nchunk, (unsigned)B);
    if (subsampling == 0)
        hipLaunchKernelGGL(jpeg_enc_blocks_kernel<0>, gblocks, dim3(256), 0, st, in, coef, H, W, (int)l.nblk, bgr ? 1 : 0, qt);
    else
        hipLaunchKernelGGL(jpeg_enc_blocks_kernel<2>, gblocks, dim3(256), 0, st, in, coef, H, W, (int)l.nblk, bgr ? 1 : 0, qt);
    HIPC(hipGetLastError());
    hipLaunchKernelGGL(jpeg_enc_len_kernel, ggrp, dim3(JPEG_ENC_GROUP), 0, st, (const short*)coef, (int)l.nblk, subsampling, boff, part);
    HIPC(hipGetLastError());
    hipLaunchKernelGGL(jpeg_enc_scan_bits_kernel, dim3((unsigned)B), dim3(256), 0, st, part, (int)l.ngrp, totbits);
    HIPC(hipGetLastError());
    hipLaunchKernelGGL(jpeg_enc_emit_kernel, ggrp, dim3(JPEG_ENC_GROUP), 0, st, (const short*)coef, (int)l.nblk, subsampling,
                       (const unsigned int*)boff, (const unsigned int*)part, (const unsigned int*)totbits, raw, (long long)l.rawcap);
    HIPC(hipGetLastError());
    hipLaunchKernelGGL(jpeg_enc_count_kernel, gchunk, dim3(256), 0, st, (const unsigned int*)raw, (long long)l.rawcap,
                       (const unsigned int*)totbits, ffpart);
    HIPC(hipGetLastError());
    hipLaunchKernelGGL(jpeg_enc_scan_ff_kernel, dim3((unsigned)B), dim3(256), 0, st, ffpart, (int)l.nchunk, (long long)l.rawcap,
                       (const unsigned int*)totbits, stride, (int*)lengths);
    HIPC(hipGetLastError());
    hipLaunchKernelGGL(jpeg_enc_scatter_kernel, gchunk, dim3(256), 0, st, (const unsigned int*)raw, (long long)l.rawcap,
                       (const unsigned int*)totbits, (const unsigned int*)ffpart, header, (const int*)lengths,
                       (unsigned char*)out, stride);
    HIPC(hipGetLastError());
    API_END
}

// Baseline JPEG decoder of the val loop's input files (csrc/jpeg_decode.hip.h).  The three host functions need no device.
int32_t ucdir_jpeg_decode_info(const uint8_t* file_host, int64_t len, int32_t* info_host) {
    if (!file_host || !info_host || len < 0) return jpeg_dec::BAD_SOI;
    jpeg_dec::Parsed P;
    const int rc = jpeg_dec::parse(file_host, len, P);
    if (rc == 0) std::memcpy(info_host, P.info, sizeof(P.info));
    return rc;
}

int64_t ucdir_jpeg_decode_pack(const uint8_t* file_host, int64_t len, uint8_t* packed_host, int64_t cap) {
    if (!file_host || !packed_host || len < 0) return -1;
    return jpeg_dec::pack(file_host, len, packed_host, cap);
}

int64_t ucdir_jpeg_decode_workspace_bytes(const int32_t* info_host) {
    if (!info_host || !jpeg_dec::info_consistent(info_host)) return -1;
    return jpeg_dec::layout(info_host).bytes;
}

// The checks and the launches of ucdir_jpeg_decode; ev: null, or five events recorded in front of the memsets and behind the
// memsets, the Huffman, the IDCT and the colour launch (ucdir_jpeg_decode_profile).  Throws.
static void jpeg_decode_run(const std::string& fn, const uint8_t* packed_dev, int64_t packed_len, const int32_t* info_host, uint8_t* out,
                            int32_t x0, int32_t y0, int32_t w, int32_t h, int32_t bgr, void* workspace, int32_t* status_dev,
                            hipStream_t st, hipEvent_t* ev) {
    using namespace jpeg_dec;
    require(packed_dev && info_host && out && workspace && status_dev, fn + ": null argument");
    require(info_consistent(info_host), fn + ": info is not what ucdir_jpeg_decode_info fills");
    require(packed_len == info_host[INFO_PACKED_BYTES], fn + ": packed_len is not the info's packed byte count");
    const int W = info_host[INFO_WIDTH], H = info_host[INFO_HEIGHT];
    require(w >= 1 && h >= 1 && x0 >= 0 && y0 >= 0 && (int64_t)x0 + w <= W && (int64_t)y0 + h <= H, fn + ": the crop must lie inside the image");
    require(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)packed_dev & 15) == 0, fn + ": packed_dev and workspace must be 16-byte aligned");
    require(((uintptr_t)status_dev & 3) == 0, fn + ": status_dev must be 4-byte aligned");
    const void* others[3] = {out, workspace, status_dev};
    const char* names[3] = {"out", "workspace", "status_dev"};
    const int device = same_device(fn, packed_dev, "packed_dev", others, names, 3);
    const Layout l = layout(info_host);
    DevGuard dg(device);
    unsigned char* ws = (unsigned char*)workspace;
    short* coef = (short*)(ws + l.coef);
    const int nblk = info_host[INFO_BLOCKS], nseg = info_host[INFO_SEGMENTS], bpm = info_host[INFO_BLOCKS_PER_MCU];
    const int hs = info_host[INFO_HS], vs = info_host[INFO_VS], ncomp = info_host[INFO_COMPONENTS];
    auto mark = [&](int i) { if (ev) HIPC(hipEventRecord(ev[i], st)); };
    mark(0);
    HIPC(hipMemsetAsync(coef, 0, (size_t)nblk * 128, st));
    HIPC(hipMemsetAsync(status_dev, 0, 4, st));
    mark(1);
    hipLaunchKernelGGL(jpeg_dec_huff_kernel, dim3((unsigned)std::min(nseg, 4096)), dim3(JPEG_DEC_THREADS), 0, st, packed_dev,
                       (unsigned int)packed_len, nseg, info_host[INFO_SUBSEQS], info_host[INFO_MCUS_X] * info_host[INFO_MCUS_Y], bpm,
                       ncomp == 1 ? 1 : hs * vs, info_host[INFO_RESTART], coef, (uint4*)(ws + l.state), (unsigned int*)(ws + l.first),
                       (int*)(ws + l.rounds), (int*)status_dev);
    HIPC(hipGetLastError());
    mark(2);
    hipLaunchKernelGGL(jpeg_dec_idct_kernel, dim3((unsigned)((nblk + 31) / 32)), dim3(256), 0, st, (const short*)coef, packed_dev, nblk,
                       bpm, hs, vs, info_host[INFO_MCUS_X], ws + l.planes, (int)l.yw, (int)l.yh, (int)l.cw, (int)l.ch);
    HIPC(hipGetLastError());
    mark(3);
    const long long npix = (long long)w * h;
    hipLaunchKernelGGL(jpeg_dec_colour_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, st, (const unsigned char*)(ws + l.planes),
                       out, W, H, ncomp, hs, vs, (int)l.yw, (int)l.yh, (int)l.cw, (int)l.ch, x0, y0, w, h, bgr ? 1 : 0);
    HIPC(hipGetLastError());
    mark(4);
}

int32_t ucdir_jpeg_decode(const uint8_t* packed_dev, int64_t packed_len, const int32_t* info_host, uint8_t* out, int32_t x0, int32_t y0,
                          int32_t w, int32_t h, int32_t bgr, void* workspace, int32_t* status_dev, void* stream) {
    API_BEGIN
    jpeg_decode_run("ucdir_jpeg_decode", packed_dev, packed_len, info_host, out, x0, y0, w, h, bgr, workspace, status_dev,
                    (hipStream_t)stream, nullptr);
    API_END
}

// The same decode with an event in front of and behind every stage; waits for the stream, then reads the four times and the
// rounds the Huffman kernel left per segment in the workspace.
int32_t ucdir_jpeg_decode_profile(const uint8_t* packed_dev, int64_t packed_len, const int32_t* info_host, uint8_t* out, int32_t x0,
                                  int32_t y0, int32_t w, int32_t h, int32_t bgr, void* workspace, int32_t* status_dev, void* stream,
                                  float* stage_ms_host, int32_t* rounds_host) {
    struct Events {
        hipEvent_t e[5] = {};
        ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
    } ev;
    API_BEGIN
    const std::string fn("ucdir_jpeg_decode_profile");
    require(stage_ms_host && rounds_host, fn + ": null argument");
    // the events belong to the device the work runs on: checked again, with everything else, by jpeg_decode_run
    require(packed_dev != nullptr, fn + ": null argument");
    DevGuard dg(same_device(fn, packed_dev, "packed_dev", nullptr, nullptr, 0));
    for (hipEvent_t& x : ev.e) HIPC(hipEventCreate(&x));
    jpeg_decode_run(fn, packed_dev, packed_len, info_host, out, x0, y0, w, h, bgr, workspace, status_dev, (hipStream_t)stream, ev.e);
    HIPC(hipEventSynchronize(ev.e[4]));
    for (int i = 0; i < 4; ++i) HIPC(hipEventElapsedTime(&stage_ms_host[i], ev.e[i], ev.e[i + 1]));
    const int nseg = info_host[jpeg_dec::INFO_SEGMENTS];
    std::vector<int32_t> r((size_t)nseg);
    HIPC(hipMemcpy(r.data(), (const unsigned char*)workspace + jpeg_dec::layout(info_host).rounds, (size_t)nseg * 4, hipMemcpyDeviceToHost));
    *rounds_host = *std::max_element(r.begin(), r.end());
    API_END
}

// Several files per call (csrc/jpeg_decode.hip.h, "several files per call").  The plan is host only and needs no device.
int64_t ucdir_jpeg_decode_batch_plan(int32_t n, const int32_t* infos_host, const int32_t* crops_host, const int64_t* packed_off_host,
                                     const int64_t* out_off_host, uint8_t* buffer_host, int64_t buffer_bytes, int64_t* workspace_bytes) {
    const std::string fn("ucdir_jpeg_decode_batch_plan: ");
    jpeg_dec::BatchSizes z;
    const char* e = jpeg_dec::batch_sizes(n, infos_host, z);
    if (!e && buffer_host) e = jpeg_dec::batch_plan(n, infos_host, crops_host, packed_off_host, out_off_host, buffer_host, buffer_bytes);
    if (e) {
        fail(fn + e);
        return -1;
    }
    if (workspace_bytes) *workspace_bytes = z.ws_bytes;
    return z.table_bytes;
}

// The checks and the launches of ucdir_jpeg_decode_batch: two memsets and three launches, whatever n.  ev as in jpeg_decode_run.
static void jpeg_decode_batch_run(const std::string& fn, const uint8_t* buffer_dev, const uint8_t* table_host, int64_t buffer_bytes,
                                  uint8_t* out, int64_t out_bytes, int32_t bgr, void* workspace, int64_t workspace_bytes,
                                  int32_t* status_dev, hipStream_t st, hipEvent_t* ev) {
    using namespace jpeg_dec;
    require(buffer_dev && table_host && out && workspace && status_dev, fn + ": null argument");
    BatchHeader h;
    std::memcpy(&h, table_host, sizeof(h));
    if (const char* e = batch_header_check(h, buffer_bytes)) throw std::runtime_error(fn + ": " + e);
    require(out_bytes >= 0 && (uint64_t)out_bytes >= h.out_bytes, fn + ": out is smaller than the table's outputs");
    require(workspace_bytes >= 0 && (uint64_t)workspace_bytes >= h.ws_bytes, fn + ": workspace is smaller than the plan's workspace_bytes");
    require(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)buffer_dev & 15) == 0, fn + ": buffer_dev and workspace must be 16-byte aligned");
    require(((uintptr_t)status_dev & 3) == 0, fn + ": status_dev must be 4-byte aligned");
    const void* others[3] = {out, workspace, status_dev};
    const char* names[3] = {"out", "workspace", "status_dev"};
    const int device = same_device(fn, buffer_dev, "buffer_dev", others, names, 3);
    DevGuard dg(device);
    unsigned char* ws = (unsigned char*)workspace;
    auto mark = [&](int i) { if (ev) HIPC(hipEventRecord(ev[i], st)); };
    mark(0);
    HIPC(hipMemsetAsync(ws, 0, (size_t)h.zero_bytes, st));                 // the coefficients and the rounds of every file
    HIPC(hipMemsetAsync(status_dev, 0, (size_t)h.n * 4, st));
    mark(1);
    hipLaunchKernelGGL(jpeg_dec_huff_batch_kernel, dim3(std::min<unsigned>(h.nitems, BATCH_HUFF_GRID)), dim3(JPEG_DEC_THREADS), 0, st,
                       buffer_dev, ws, (int*)status_dev);
    HIPC(hipGetLastError());
    mark(2);
    hipLaunchKernelGGL(jpeg_dec_idct_batch_kernel, dim3(h.idct_wgs), dim3(256), 0, st, buffer_dev, ws);
    HIPC(hipGetLastError());
    mark(3);
    hipLaunchKernelGGL(jpeg_dec_colour_batch_kernel, dim3(h.colour_wgs), dim3(256), 0, st, buffer_dev, (const unsigned char*)ws, out,
                       bgr ? 1 : 0);
    HIPC(hipGetLastError());
    mark(4);
}

int32_t ucdir_jpeg_decode_batch(const uint8_t* buffer_dev, const uint8_t* table_host, int64_t buffer_bytes, uint8_t* out, int64_t out_bytes,
                                int32_t bgr, void* workspace, int64_t workspace_bytes, int32_t* status_dev, void* stream) {
    API_BEGIN
    jpeg_decode_batch_run("ucdir_jpeg_decode_batch", buffer_dev, table_host, buffer_bytes, out, out_bytes, bgr, workspace, workspace_bytes,
                          status_dev, (hipStream_t)stream, nullptr);
    API_END
}

// The batch decode with an event in front of and behind every stage; waits, then reads the four times and, in one copy, the rounds
// of every segment of the batch, of which every file gets its largest.
int32_t ucdir_jpeg_decode_batch_profile(const uint8_t* buffer_dev, const uint8_t* table_host, int64_t buffer_bytes, uint8_t* out,
                                        int64_t out_bytes, int32_t bgr, void* workspace, int64_t workspace_bytes, int32_t* status_dev,
                                        void* stream, float* stage_ms_host, int32_t* rounds_host) {
    struct Events {
        hipEvent_t e[5] = {};
        ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
    } ev;
    API_BEGIN
    using namespace jpeg_dec;
    const std::string fn("ucdir_jpeg_decode_batch_profile");
    require(stage_ms_host && rounds_host && buffer_dev && table_host, fn + ": null argument");
    DevGuard dg(same_device(fn, buffer_dev, "buffer_dev", nullptr, nullptr, 0));
    for (hipEvent_t& x : ev.e) HIPC(hipEventCreate(&x));
    jpeg_decode_batch_run(fn, buffer_dev, table_host, buffer_bytes, out, out_bytes, bgr, workspace, workspace_bytes, status_dev,
                          (hipStream_t)stream, ev.e);
    HIPC(hipEventSynchronize(ev.e[4]));
    for (int i = 0; i < 4; ++i) HIPC(hipEventElapsedTime(&stage_ms_host[i], ev.e[i], ev.e[i + 1]));
    BatchHeader h;
    std::memcpy(&h, table_host, sizeof(h));
    std::vector<BatchFile> files(h.n);
    std::memcpy(files.data(), table_host + sizeof(BatchHeader), (size_t)h.n * sizeof(BatchFile));
    const uint64_t r0 = files[0].rounds_off;                               // the rounds of all files stand together, file 0's first
    require(r0 <= h.zero_bytes && (h.zero_bytes - r0) % 4 == 0, fn + ": table_host holds no rounds region");
    std::vector<int32_t> r((size_t)((h.zero_bytes - r0) / 4));
    HIPC(hipMemcpy(r.data(), (const unsigned char*)workspace + r0, r.size() * 4, hipMemcpyDeviceToHost));
    for (uint32_t k = 0; k < h.n; ++k) {
        const uint64_t at = (files[k].rounds_off - r0) / 4;
        require(files[k].rounds_off >= r0 && files[k].nseg >= 1 && at + (uint64_t)files[k].nseg <= r.size(), fn + ": table_host holds a rounds slice outside its region");
        rounds_host[k] = *std::max_element(r.begin() + at, r.begin() + at + files[k].nseg);
    }
    API_END
}

// Pillow-exact resampling of the super-resolution val task (csrc/resample.hip.h).  Table layout in the workspace: per changing
// axis out_size * ksize coefficients then out_size (min, count) pairs, horizontal axis first; 16-byte rounded; then the
// intermediate image.
static const char* resample_check(int32_t B, int32_t Hin, int32_t Win, int32_t Hout, int32_t Wout, int32_t filter) {
    if (B < 1 || Hin < 1 || Win < 1 || Hout < 1 || Wout < 1) return "sizes must be at least 1";
    if (filter < 0 || filter > 3) return "unknown filter (0 box, 1 bilinear, 2 bicubic, 3 Lanczos)";
    if (Hin > 65536 || Win > 65536 || Hout > 65536 || Wout > 65536) return "sides above 65536 are not supported";
    if ((int64_t)B * std::max(Hin, Hout) >= (1LL << 31)) return "more than 2^31 - 1 rows";
    if ((Win != Wout && resample::ksize_of(Win, Wout, filter) > RESAMPLE_MAX_KSIZE) ||
        (Hin != Hout && resample::ksize_of(Hin, Hout, filter) > RESAMPLE_MAX_KSIZE))
        return "ratio too large: the filter would span more than 129 taps (ksize cap)";
    return nullptr;
}

static int64_t resample_table_ints(int32_t in_size, int32_t out_size, int32_t filter_ksize) {
    return in_size == out_size ? 0 : (int64_t)out_size * (filter_ksize + 2);
}

int32_t ucdir_resample_coeffs(int32_t in_size, int32_t out_size, int32_t filter, int32_t* kk, int32_t* bounds, int32_t* ksize) {
    API_BEGIN
    const std::string w("ucdir_resample_coeffs");
    require(in_size >= 1 && out_size >= 1, w + ": sizes must be at least 1");
    require(filter >= 0 && filter <= 3, w + ": unknown filter (0 box, 1 bilinear, 2 bicubic, 3 Lanczos)");
    require(ksize, w + ": null argument");
    require((kk == nullptr) == (bounds == nullptr), w + ": kk and bounds must both be given or both be null");
    const int ks = resample::ksize_of(in_size, out_size, filter);
    require(ks <= (1 << 20), w + ": ratio too large");
    *ksize = ks;
    if (kk) resample::coeffs(in_size, out_size, filter, ks, kk, bounds);
    API_END
}

int64_t ucdir_resample_workspace_bytes(int32_t B, int32_t Hin, int32_t Win, int32_t Hout, int32_t Wout) {
    if (resample_check(B, Hin, Win, Hout, Wout, 0)) return -1;
    // sized for any filter a call accepts: the widest one, Lanczos, up to the tap cap
    const int64_t ints = resample_table_ints(Win, Wout, std::min(resample::ksize_of(Win, Wout, 3), RESAMPLE_MAX_KSIZE)) +
                         resample_table_ints(Hin, Hout, std::min(resample::ksize_of(Hin, Hout, 3), RESAMPLE_MAX_KSIZE));
    const int64_t tmp = (Win != Wout && Hin != Hout) ? (int64_t)B * Hin * Wout * 3 : 0;
    return std::max<int64_t>((ints * 4 + 15) / 16 * 16 + tmp, 16);
}

int32_t ucdir_resample(const uint8_t* in, uint8_t* out, int32_t B, int32_t Hin, int32_t Win, int32_t Hout, int32_t Wout,
                       int32_t filter, void* workspace, void* stream) {
    API_BEGIN
    const std::string w("ucdir_resample");
    require(in && out && workspace, w + ": null argument");
    const char* bad = resample_check(B, Hin, Win, Hout, Wout, filter);
    require(!bad, w + ": " + (bad ? bad : ""));
    require(in != out, w + ": in and out must differ");
    require(((uintptr_t)workspace & 15) == 0, w + ": workspace must be 16-byte aligned");
    const void* others[2] = {out, workspace};
    const char* names[2] = {"out", "workspace"};
    const int device = same_device(w, in, "in", others, names, 2);
    const bool horiz = Win != Wout, vert = Hin != Hout;
    const int ksh = horiz ? resample::ksize_of(Win, Wout, filter) : 0, ksv = vert ? resample::ksize_of(Hin, Hout, filter) : 0;
    const int64_t ints_h = resample_table_ints(Win, Wout, ksh), ints_v = resample_table_ints(Hin, Hout, ksv);
    DevGuard dg(device);
    hipStream_t st = (hipStream_t)stream;
    if (!horiz && !vert) {                                      // Pillow's resize to the same size: a copy
        HIPC(hipMemcpyAsync(out, in, (size_t)B * Hin * Win * 3, hipMemcpyDeviceToDevice, st));
        return 0;
    }
    // The tables go up from pageable host memory: such a copy has left the host buffer when hipMemcpyAsync returns.
    std::vector<int32_t> tab((size_t)(ints_h + ints_v));
    int32_t* const d_tab = (int32_t*)workspace;
    if (horiz) resample::coeffs(Win, Wout, filter, ksh, tab.data(), tab.data() + (size_t)Wout * ksh);
    if (vert) resample::coeffs(Hin, Hout, filter, ksv, tab.data() + ints_h, tab.data() + ints_h + (size_t)Hout * ksv);
    HIPC(hipMemcpyAsync(d_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, st));
    unsigned char* const tmp = (unsigned char*)workspace + ((ints_h + ints_v) * 4 + 15) / 16 * 16;
    const unsigned char* vsrc = in;
    if (horiz) {
        const long long rows = (long long)B * Hin;
        const dim3 grid((unsigned)((rows + RESAMPLE_RY - 1) / RESAMPLE_RY), (unsigned)((Wout + RESAMPLE_TX - 1) / RESAMPLE_TX));
        hipLaunchKernelGGL(resample_h_kernel, grid, dim3(RESAMPLE_TX * 3), (size_t)RESAMPLE_TX * (ksh + 2) * 4, st, in,
                           vert ? tmp : out, (const int*)d_tab, (const int*)d_tab + (size_t)Wout * ksh, rows, Win, Wout, ksh);
        HIPC(hipGetLastError());
        vsrc = tmp;
    }
    if (vert) {
        const int N = Wout * 3;
        hipLaunchKernelGGL(resample_v_kernel, dim3((unsigned)(B * Hout), (unsigned)((N + 255) / 256)), dim3(256), 0, st, vsrc, out,
                           (const int*)d_tab + ints_h, (const int*)d_tab + ints_h + (size_t)Hout * ksv, Hin, Hout, N, ksv);
        HIPC(hipGetLastError());
    }
    API_END
}

// NIQE features of the val loop (csrc/niqe.hip.h).  Workspace: the MSCN planes of both scales per image (5/4 Hc Wc floats, used when
// the caller passes no buffer of its own), then the half-size Y planes (1/4 Hc Wc floats per image); Hc x Wc = the crop to whole
// 96 x 96 blocks.
int64_t ucdir_niqe_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W) {
    if (B <= 0 || H <= 0 || W <= 0 || (C != 1 && C != 3)) return -1;
    const int64_t nblk = (int64_t)(H / NQ_BLOCK) * (W / NQ_BLOCK);
    if (nblk < 1) return -1;
    return (int64_t)B * nblk * NQ_BLOCK * NQ_BLOCK * 6 / 4 * (int64_t)sizeof(float);
}

int32_t ucdir_niqe_features(const float* x, int64_t x_sn, int64_t x_sc, int64_t x_sh, int32_t B, int32_t C, int32_t H, int32_t W,
                            const double* window49, const double* tables, double* feats, float* mscn_or_null, void* workspace,
                            void* stream) {
    API_BEGIN
    const std::string w("ucdir_niqe_features");
    require(x && window49 && tables && feats && workspace, w + ": null argument");
    require(C == 1 || C == 3, w + ": C must be 1 or 3");
    require(B > 0 && B <= 65535, w + ": B must lie in 1..65535");
    require(H >= NQ_BLOCK && W >= NQ_BLOCK, w + ": H and W must be at least 96");
    const int nh = H / NQ_BLOCK, nw = W / NQ_BLOCK, Hc = nh * NQ_BLOCK, Wc = nw * NQ_BLOCK;
    const long long nblk = (long long)nh * nw, plane = (long long)Hc * Wc;
    require(plane / (NQ_T / 2 * NQ_T / 2) <= 0x7fffffffLL, w + ": image too large");
    require(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)feats & 7) == 0 && ((uintptr_t)tables & 7) == 0 &&
            ((uintptr_t)mscn_or_null & 3) == 0, w + ": workspace, tables and feats must be 8-byte aligned, mscn 4-byte");
    const void* others[4] = {tables, feats, workspace, mscn_or_null};
    const char* names[4] = {"tables", "feats", "workspace", "mscn"};
    const int device = same_device(w, x, "x", others, names, 4);
    NiqeWindow win;
    for (int k = 0; k < 49; ++k) win.w[k] = window49[k];
    DevGuard dg(device);
    hipStream_t st = (hipStream_t)stream;
    float* mscn = mscn_or_null ? mscn_or_null : (float*)workspace;
    float* y2 = (float*)workspace + (long long)B * plane * 5 / 4;
    const long long mscn_sn = plane * 5 / 4;
    hipLaunchKernelGGL(niqe_mscn_kernel<1>, dim3((unsigned)(plane / (NQ_T * NQ_T)), (unsigned)B), dim3(256), 0, st, x, (long long)x_sn,
                       (long long)x_sc, (long long)x_sh, C, Hc, Wc, win, (const float*)nullptr, mscn, mscn_sn, y2);
    HIPC(hipGetLastError());
    hipLaunchKernelGGL(niqe_mscn_kernel<2>, dim3((unsigned)(plane / 4 / (NQ_T * NQ_T)), (unsigned)B), dim3(256), 0, st,
                       (const float*)nullptr, 0LL, 0LL, 0LL, 1, Hc / 2, Wc / 2, win, (const float*)y2, mscn + plane, mscn_sn,
                       (float*)nullptr);
    HIPC(hipGetLastError());
    for (int scale = 1; scale <= 2; ++scale) {
        hipLaunchKernelGGL(niqe_block_kernel, dim3((unsigned)nblk, (unsigned)B), dim3(256), 0, st,
                           (const float*)(scale == 1 ? mscn : mscn + plane), mscn_sn, Wc / scale, NQ_BLOCK / scale, nh, (int)nblk, scale,
                           tables, feats);
        HIPC(hipGetLastError());
    }
    API_END
}

// Degradation operators of the real-world SR val task (csrc/realsr.hip.h).
static void filter2d_check(const std::string& w, int32_t B, int32_t C, int32_t H, int32_t W, int32_t k) {
    require(B > 0 && C > 0 && H > 0 && W > 0, w + ": bad shape (B, C, H and W at least 1)");
    require((int64_t)B * C <= 65535, w + ": more than 65535 planes (B * C)");
    require(k >= 1 && (k & 1) == 1, w + ": the kernel size must be odd");
    require(k <= F2D_KMAX, w + ": the kernel size must be at most 21");
    require(H > k / 2 && W > k / 2, w + ": the reflect pad k / 2 must be smaller than H and W");
    require((int64_t)((H + F2D_TH - 1) / F2D_TH) * ((W + F2D_TW - 1) / F2D_TW) < (1LL << 31), w + ": image too large");
}

int32_t ucdir_filter2d(const float* x, const float* kernels, float* y, int32_t B, int32_t C, int32_t H, int32_t W, int32_t k,
                       int32_t per_sample, void* stream) {
    API_BEGIN
    const std::string w("ucdir_filter2d");
    filter2d_check(w, B, C, H, W, k);
    require(x && kernels && y, w + ": null argument");
    require(x != y, w + ": x and y must not alias");
    const void* others[2] = {kernels, y};
    const char* names[2] = {"kernels", "y"};
    DevGuard dg(same_device(w, x, "x", others, names, 2));
    const unsigned tiles = (unsigned)(((H + F2D_TH - 1) / F2D_TH) * ((W + F2D_TW - 1) / F2D_TW));
    hipLaunchKernelGGL(filter2d_kernel<0>, dim3(tiles, (unsigned)(B * C)), dim3(256), 0, (hipStream_t)stream, x,
                       (const unsigned char*)nullptr, kernels, UsmGauss{}, y, (unsigned char*)nullptr, C, H, W, k, per_sample ? 1 : 0,
                       0.f, 0.f);
    HIPC(hipGetLastError());
    API_END
}

// cv2.getGaussianKernel(k, sigma = 0) in float64: the fixed tables OpenCV keeps for k <= 7, else sigma = 0.3 ((k - 1) / 2 - 1) + 0.8
static void usm_gauss(int k, double* g) {
    static const double small[4][7] = {{1.0}, {0.25, 0.5, 0.25}, {0.0625, 0.25, 0.375, 0.25, 0.0625},
                                       {0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125}};
    if (k <= 7) {
        for (int i = 0; i < k; ++i) g[i] = small[k >> 1][i];
        return;
    }
    const double sigma = 0.3 * ((k - 1) * 0.5 - 1.0) + 0.8, s2 = -0.5 / (sigma * sigma);
    double sum = 0.0;
    for (int i = 0; i < k; ++i) {
        const double d = i - (k - 1) * 0.5;
        g[i] = std::exp(s2 * d * d);
        sum += g[i];
    }
    for (int i = 0; i < k; ++i) g[i] *= 1.0 / sum;
}

int64_t ucdir_usm_sharp_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return -1;
    return (int64_t)B * C * H * W;                        // the mask, one byte per element
}

int32_t ucdir_usm_sharp(const float* x, float* y, int32_t B, int32_t C, int32_t H, int32_t W, int32_t radius, float weight,
                        float threshold, void* workspace, void* stream) {
    API_BEGIN
    const std::string w("ucdir_usm_sharp");
    require(radius >= 1, w + ": radius must be at least 1");
    const int k = radius | 1;                            // an even radius takes the next odd size, as the reference
    filter2d_check(w, B, C, H, W, k);
    require(x && y && workspace, w + ": null argument");
    require(x != y, w + ": x and y must not alias");
    const void* others[2] = {y, workspace};
    const char* names[2] = {"y", "workspace"};
    DevGuard dg(same_device(w, x, "x", others, names, 2));
    UsmGauss gs{};
    usm_gauss(k, gs.g);
    const dim3 grid((unsigned)(((H + F2D_TH - 1) / F2D_TH) * ((W + F2D_TW - 1) / F2D_TW)), (unsigned)(B * C));
    unsigned char* mask = (unsigned char*)workspace;
    hipLaunchKernelGGL(filter2d_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, x, (const unsigned char*)nullptr,
                       (const float*)nullptr, gs, y, mask, C, H, W, k, 0, weight, threshold);
    HIPC(hipGetLastError());
    hipLaunchKernelGGL(filter2d_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, x, (const unsigned char*)mask,
                       (const float*)nullptr, gs, y, (unsigned char*)nullptr, C, H, W, k, 0, weight, threshold);
    HIPC(hipGetLastError());
    API_END
}

int32_t ucdir_diffjpeg(const float* x, float* y, const float* factors, int32_t B, int32_t H, int32_t W, void* stream) {
    API_BEGIN
    const std::string w("ucdir_diffjpeg");
    require(B > 0 && B <= 65535 && H > 0 && W > 0, w + ": bad shape (B in 1..65535, H and W at least 1)");
    require((int64_t)((H + 15) / 16) * ((W + 15) / 16) < (1LL << 31), w + ": image too large");
    require(x && y && factors, w + ": null argument");
    const void* others[2] = {y, factors};
    const char* names[2] = {"y", "factors"};
    DevGuard dg(same_device(w, x, "x", others, names, 2));
    DiffJpegTables t;
    const double pi = 3.14159265358979323846;
    for (int i = 0; i < 8; ++i)
        for (int u = 0; u < 8; ++u) t.cosv[i][u] = std::cos((2 * i + 1) * u * pi / 16);
    for (int u = 0; u < 8; ++u)
        for (int v = 0; v < 8; ++v) {
            const double au = u ? 1.0 : 1.0 / std::sqrt(2.0), av = v ? 1.0 : 1.0 / std::sqrt(2.0);
            t.table[0][u * 8 + v] = (float)std_luma[v * 8 + u];     // the reference transposes the luma table
            t.table[1][u * 8 + v] = (u < 4 && v < 4) ? (float)std_chroma4[v * 4 + u] : 99.f;
            t.scale[u * 8 + v] = (float)(au * av * 0.25);
            t.alpha[u * 8 + v] = (float)(au * av);
        }
    const float fwd[3][3] = {{0.299f, 0.587f, 0.114f}, {-0.168736f, -0.331264f, 0.5f}, {0.5f, -0.418688f, -0.081312f}};
    const float inv[3][3] = {{1.f, 0.f, 1.402f}, {1.f, -0.344136f, -0.714136f}, {1.f, 1.772f, 0.f}};
    std::memcpy(t.fwd, fwd, sizeof fwd);
    std::memcpy(t.inv, inv, sizeof inv);
    hipLaunchKernelGGL(diffjpeg_kernel, dim3((unsigned)(((H + 15) / 16) * ((W + 15) / 16)), (unsigned)B), dim3(256), 0,
                       (hipStream_t)stream, x, y, factors, H, W, t);
    HIPC(hipGetLastError());
    API_END
}

}  // extern "C"
