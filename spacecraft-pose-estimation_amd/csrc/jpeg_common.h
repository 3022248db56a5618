// What the JPEG decoder (jpeg_decode.hip) and the JPEG encoder (jpeg_encode.hip) must agree on for a stream to pass from one to
// the other byte for byte: the frame in MCUs and blocks, the zig-zag order, the block -> component mapping inside an MCU and the
// constants of libjpeg's ISLOW DCT pair.  api.cpp bounds its batches with jpeg_blocks().
#pragma once
#include "common.h"

namespace scpose {

// The frame of one image in scan order.  hs: luma sampling factor in both directions (2 for 4:2:0); an MCU holds ycount = hs * hs
// Y blocks followed by one Cb and one Cr block (bpm in all; gray: the one Y block) and covers 8 hs x 8 hs pixels.
struct JpegFrame {
  int32_t hs, ycount, bpm, mcus_x, mcus_y, n_mcus, n_blocks;
};
inline JpegFrame jpeg_frame(int h, int w, int mode) {
  JpegFrame f{};
  f.hs = mode == SCPOSE_JPEG_420 ? 2 : 1;
  f.ycount = f.hs * f.hs;
  f.bpm = mode == SCPOSE_JPEG_GRAY ? 1 : f.ycount + 2;
  f.mcus_x = (w + 8 * f.hs - 1) / (8 * f.hs);
  f.mcus_y = (h + 8 * f.hs - 1) / (8 * f.hs);
  f.n_mcus = f.mcus_x * f.mcus_y;
  f.n_blocks = f.n_mcus * f.bpm;
  return f;
}
inline int64_t jpeg_blocks(int h, int w, int mode) { return jpeg_frame(h, w, mode).n_blocks; }

// jpeg_natural_order: natural index of the k-th coefficient in zig-zag order, as a constant expression and as a device lookup
__constant__ constexpr uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                              41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                              30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// Blocks and components inside an MCU.  Component 0 is Y, 1 and 2 are Cb and Cr; a component's blocks are consecutive.
// the component that block blk of an MCU belongs to.  The expression is a macro for the decoder's walk(): an inlined function is
// simplified on its own before it meets the loop around it, and the loop then compiles to other instructions than it had
#define SCP_MCU_COMP_INDEX(blk, ycount) ((blk) < (ycount) ? 0 : (blk) - (ycount) + 1)
__device__ __forceinline__ int mcu_comp_index(int blk, int ycount) { return SCP_MCU_COMP_INDEX(blk, ycount); }
// a component, its first block in the MCU and the blocks it has there
struct McuComp {
  int comp, first, count;
};
__device__ __forceinline__ McuComp mcu_comp(int comp, int ycount) {
  McuComp m;
  m.comp = comp;
  m.count = comp == 0 ? ycount : 1;
  m.first = comp == 0 ? 0 : ycount + comp - 1;
  return m;
}
__device__ __forceinline__ McuComp mcu_comp_of_block(int blk, int ycount) { return mcu_comp(mcu_comp_index(blk, ycount), ycount); }

// jfdctint.c / jidctint.c, CONST_BITS 13, PASS1_BITS 2: FIX(0.298631336) ... FIX(3.072711026)
constexpr int32_t F0298 = 2446, F0390 = 3196, F0541 = 4433, F0765 = 6270, F0899 = 7373, F1175 = 9633, F1501 = 12299, F1847 = 15137,
                  F1961 = 16069, F2053 = 16819, F2562 = 20995, F3072 = 25172;

}  // namespace scpose
