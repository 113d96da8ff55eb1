// Work items of the image-load kernel (image_load.hip): the image constants, the source kinds, the destinations, the item count and the map
// from a work-item index to its run of pixels, its source offset and its destination offset, as plain functions of plain values.  No
// HIP type and no header is used here, so a host compiler reads this file on its own (tools/image_items_check.cpp walks every item
// without a GPU).
#pragma once

#if defined(__HIP__) || defined(__HIPCC__)
#define DYT_ITEM_HD __host__ __device__
#else
#define DYT_ITEM_HD
#endif

namespace dyt {

constexpr int IMG = 224, PS = 16, GRID_P = IMG / PS;   // 14 x 14 patches of 16 x 16
constexpr unsigned long long PLANE = (unsigned long long)IMG * IMG;

// Source kinds (the src_kind values of dyt_mix_images / dyt_erase_images).  A work item owns one run of consecutive pixels of one image
// row; a row of 224 pixels is a whole number of either run, so a run never crosses a row.
//   fp32 [B,3,224,224]: 4 pixels of one channel (one 16-byte load);  uint8 [B,3,224,224]: 16 pixels of one channel (one 16-byte load);
//   uint8 [B,224,224,3]: 16 pixels x 3 channels, 48 contiguous bytes (three 16-byte loads)
constexpr int IMAGE_SRC_F32 = 0, IMAGE_SRC_U8 = 1, IMAGE_SRC_U8_NHWC = 2;
// Destinations.  The embedding operand (the EPI_EMBED GEMM's A, fp32 or 16-bit): out[(b*196 + py*14 + px)*768 + c*256 + i*16 + j] =
// pixel [b][c][py*16+i][px*16+j];  fp32 planes [B,3,224,224].
constexpr int IMAGE_DST_OPERAND_F32 = 0, IMAGE_DST_OPERAND_16 = 1, IMAGE_DST_PLANES = 2;

DYT_ITEM_HD constexpr int image_run(int kind) { return kind == IMAGE_SRC_F32 ? 4 : 16; }            // pixels of an item's run
DYT_ITEM_HD constexpr int image_item_channels(int kind) { return kind == IMAGE_SRC_U8_NHWC ? 3 : 1; }   // channels an item covers
// elements between an item's channels in the destination (IMAGE_SRC_U8_NHWC: channel c of the run goes to dst + c * this)
DYT_ITEM_HD constexpr unsigned long long image_channel_stride(bool planes) { return planes ? PLANE : (unsigned long long)PS * PS; }

// The items of a batch, the same number for either destination: every pixel of every channel lies in one run.
DYT_ITEM_HD constexpr unsigned long long image_item_count(int kind, int batch) {
    return (unsigned long long)batch * (3 * PLANE / (unsigned long long)(image_run(kind) * image_item_channels(kind)));
}

struct ImageItem {
    int b, c, y, x0;               // image; channel (IMAGE_SRC_U8_NHWC: 0, the first of the three); row; first column of the run
    unsigned long long src, dst;   // element offsets: the run within source image b; the run's (first channel's) elements in the destination
};

// Consecutive items write consecutive 16-byte (fp32 source) or 64-byte groups of the destination, so a wave's stores are contiguous.
// Operand: the items enumerate (row, k4) / (row, c, i) / (row, i) with row = b * 196 + patch.  Planes: linear groups of the image.
template <int KIND, bool PLANES>
DYT_ITEM_HD inline ImageItem image_item(unsigned long long idx) {
    constexpr int N = image_run(KIND);
    ImageItem t;
    if (PLANES) {
        const unsigned long long per = image_item_count(KIND, 1);
        t.b = (int)(idx / per);
        const unsigned long long at = (idx - (unsigned long long)t.b * per) * N;   // channel-major: element within the image; channels-last: pixel
        const int pix = (int)(KIND == IMAGE_SRC_U8_NHWC ? at : at % PLANE);
        t.c = KIND == IMAGE_SRC_U8_NHWC ? 0 : (int)(at / PLANE);
        t.y = pix / IMG;
        t.x0 = pix - t.y * IMG;
        t.src = KIND == IMAGE_SRC_U8_NHWC ? at * 3 : at;
        t.dst = KIND == IMAGE_SRC_U8_NHWC ? (unsigned long long)t.b * 3 * PLANE + pix : idx * N;
    } else {
        // k: the item's first column of the operand row, c * 256 + i * 16 + j
        constexpr int PER_ROW = 3 * PS * PS / (N * image_item_channels(KIND));
        const int k = (int)(idx % PER_ROW) * N;
        const unsigned long long row = idx / PER_ROW;
        const int p = (int)(row % (GRID_P * GRID_P));
        const int py = p / GRID_P, px = p - py * GRID_P;
        t.b = (int)(row / (GRID_P * GRID_P));
        t.c = k >> 8;
        t.y = py * PS + ((k >> 4) & 15);
        t.x0 = px * PS + (k & 15);
        t.src = KIND == IMAGE_SRC_U8_NHWC ? ((unsigned long long)t.y * IMG + t.x0) * 3 : ((unsigned long long)t.c * IMG + t.y) * IMG + t.x0;
        t.dst = row * (3 * PS * PS) + k;
    }
    return t;
}

}  // namespace dyt
