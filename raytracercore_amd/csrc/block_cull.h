// block_cull.h -- which 8x8 pixel blocks of a path-tracing launch can see the scene (block_cull.cpp).
// Host only, fp64, no HIP calls.
#pragma once
#include <cstdint>
#include <vector>

#include "rt_internal.h"

namespace rtc {

// The pixels of a launch as PathParams names them: tile pixel (px, py), px < w, py < h, is frame
// pixel (x0 + px, y0 + py), or with band > 0 frame row
// y0 + ((py / band) * band_stride + band_offset) * band + py % band.
struct CullWindow {
    int x0, y0, w, h;
    int band, band_stride, band_offset;
};

// dead[by * blocks_x + bx] = 1 when no sample of any real pixel of that block can give a camera ray
// that meets the scene bound (blocks_x = ceil(w / 8), ceil(h / 8) block rows); returns the number of
// live blocks.  n_planes: the scene's planes, which lie outside the bound.  Every block is live when
// the proof is not available (block_cull.cpp says when).
int cull_blocks(const CameraF& cam, const SceneBound& bound, int n_planes, const CullWindow& win,
                std::vector<unsigned char>& dead);

// The first bounce's unit masks: masks[i], for live block i of `dead` in its order, has bit u clear
// exactly when the block's sample rectangle is disjoint from the projected hull of unit u's box
// (n_units boxes, 3 floats each in unit_lo / unit_hi, padded as the bound is: FlatUnits), by the cull's
// own test and margins.  A unit whose box the proof does not serve (not wholly ahead of the camera
// plane, or past the error bound) keeps its bit in every block.  false, and every mask all ones: the
// cull itself has no proof for this camera.
bool unit_masks(const CameraF& cam, const SceneBound& bound, int n_units, const float* unit_lo, const float* unit_hi,
                const CullWindow& win, const std::vector<unsigned char>& dead, std::vector<uint64_t>& masks);

// Real pixels (px < w, py < h) of the dead blocks.
uint64_t dead_pixels(const CullWindow& win, const std::vector<unsigned char>& dead);

} // namespace rtc
