// Host-side dispatch shared by conv3d.hip and conv3d_spatial.hip.
#pragma once
#include <torch/extension.h>

#include <vector>

// conv3d_spatial.hip: one-pass parity stride-2 dgrad
torch::Tensor conv3d_dgrad_s2_spatial(torch::Tensor go, torch::Tensor w,
                                      std::vector<int64_t> in_shape);

// Sub-grid planes (the half-resolution H x W plane of one parity class) the
// depth-blocked <OWT 8, DT 2> instance of conv3d_dgrad_s2_sp_kernel covers
// whole: one block owns the 8 x 8 plane at two sub-grid depths, one wave
// row per depth. Mirrors the forward's TW == 8 && TH <= 8. A short plane
// (hq < 8) leaves 8 - hq rows of each tile masked; the alternative, the
// <8> instance, would mask 16 - hq.
static inline bool s2_dgrad_depth_blocked(int hq, int wq) {
  return wq == 8 && hq <= 8;
}

// Stride-2 dgrads that conv3d_dgrad forwards to the one-pass kernel: the
// small sub-grid planes the Python route (hsub * wsub >= 128) sends to the
// igemm entry point, at the one-pass kernel's channel floor (a 32-co tile
// is one k-step). Everything else the igemm entry receives stays on the
// parity igemm kernel.
static inline bool s2_dgrad_takes_onepass(int cout, int h, int w) {
  return cout >= 32 && s2_dgrad_depth_blocked((h + 1) / 2, (w + 1) / 2);
}
