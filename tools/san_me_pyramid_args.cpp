// Host-side sanitiser check of the argument checking of lsfa_luma_pyramid, lsfa_mv_refine_chain, lsfa_mv_estimate and lsfa_mv_estimate_chain
// (the rules the searches share, me_common.h, through every export that uses them): every refusal happens before any launch, so this runs
// without a GPU.  Build and run (address + undefined-behaviour sanitisers on the host code only):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -I include -I lsfa_amd/csrc \
//         tools/san_me_pyramid_args.cpp lsfa_amd/csrc/me_pyramid.hip lsfa_amd/csrc/me.hip lsfa_amd/csrc/runtime.hip -o san_me_pyramid_args && \
//         ./san_me_pyramid_args
// Pointers are never dereferenced by a refused call; they only need the right alignment.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "lsfa_hip.h"

static int failures = 0, checks = 0;

static void refused(int rc, const char* want, const char* what) {
  const char* msg = lsfa_last_error();
  ++checks;
  if (rc == LSFA_OK || !msg || !strstr(msg, want)) {
    printf("FAIL %s: rc %d, message %s (wanted \"%s\")\n", what, rc, msg ? msg : "(null)", want);
    ++failures;
  }
}

int main(void) {
  alignas(16) static unsigned char planes[64];
  alignas(16) static int rows[64];
  unsigned char* p = planes;
  const int W = 96, H = 64;
  const long long S = (long long)W * H, S1 = S / 4, S2 = S / 16;
  // lsfa_luma_pyramid
  refused(lsfa_luma_pyramid(p, S, 3, W, H, 0, p, S1, p, S2, nullptr), "levels 0", "pyramid levels 0");
  refused(lsfa_luma_pyramid(p, S, 3, W, H, 3, p, S1, p, S2, nullptr), "levels 3", "pyramid levels 3");
  refused(lsfa_luma_pyramid(nullptr, S, 3, W, H, 2, p, S1, p, S2, nullptr), "NULL", "pyramid luma NULL");
  refused(lsfa_luma_pyramid(p, S, 3, W, H, 2, nullptr, S1, p, S2, nullptr), "NULL", "pyramid level1 NULL");
  refused(lsfa_luma_pyramid(p, S, 3, W, H, 2, p, S1, nullptr, S2, nullptr), "NULL", "pyramid level2 NULL");
  refused(lsfa_luma_pyramid(p, S, 3, 0, H, 2, p, S1, p, S2, nullptr), "bad frame size", "pyramid width 0");
  refused(lsfa_luma_pyramid(p, S, 3, 1 << 16, 1 << 16, 2, p, S1, p, S2, nullptr), "bad frame size", "pyramid 2^32 pixels");
  refused(lsfa_luma_pyramid(p, S, 0, W, H, 2, p, S1, p, S2, nullptr), "planes", "pyramid 0 planes");
  refused(lsfa_luma_pyramid(p, S, 65536, W, H, 2, p, S1, p, S2, nullptr), "planes", "pyramid 65536 planes");
  refused(lsfa_luma_pyramid(p, S - 1, 3, W, H, 2, p, S1, p, S2, nullptr), "plane stride", "pyramid short stride");
  refused(lsfa_luma_pyramid(p, S, 3, W, H, 2, p, S1 - 4, p, S2, nullptr), "level 1 stride", "pyramid short level 1 stride");
  refused(lsfa_luma_pyramid(p, S, 3, W, H, 2, p, S1 + 2, p, S2, nullptr), "multiple of 4", "pyramid level 1 stride + 2");
  refused(lsfa_luma_pyramid(p, S, 3, W, H, 2, p, S1, p, S2 + 1, nullptr), "level 2 stride", "pyramid level 2 stride + 1");
  refused(lsfa_luma_pyramid(p, S, 3, W, H, 2, p, -S1, p, S2, nullptr), "level 1 stride", "pyramid negative level 1 stride");
  refused(lsfa_luma_pyramid(p, S, 3, W, H, 2, p + 2, S1, p, S2, nullptr), "4-byte aligned", "pyramid level1 misaligned");
  refused(lsfa_luma_pyramid(p, S, 3, W, H, 2, p, S1, p + 1, S2, nullptr), "4-byte aligned", "pyramid level2 misaligned");
  // lsfa_mv_refine_chain
  refused(lsfa_mv_refine_chain(nullptr, S, 1, 2, W, H, rows, 2, 4, 0, rows, nullptr, nullptr), "NULL", "refine luma NULL");
  refused(lsfa_mv_refine_chain(p, S, 1, 2, W, H, nullptr, 2, 4, 0, rows, nullptr, nullptr), "NULL", "refine parents NULL");
  refused(lsfa_mv_refine_chain(p, S, 1, 2, W, H, rows, 2, 4, 0, nullptr, nullptr, nullptr), "NULL", "refine mvs NULL");
  refused(lsfa_mv_refine_chain(p, S, 1, 2, W, -1, rows, 2, 4, 0, rows, nullptr, nullptr), "bad frame size", "refine height -1");
  refused(lsfa_mv_refine_chain(p, S, 1, 2, W, H, rows, 0, 4, 0, rows, nullptr, nullptr), "refine 0", "refine 0");
  refused(lsfa_mv_refine_chain(p, S, 1, 2, W, H, rows, 4, 4, 0, rows, nullptr, nullptr), "refine 4", "refine 4");
  refused(lsfa_mv_refine_chain(p, S, 1, 2, W, H, rows, 2, -1, 0, rows, nullptr, nullptr), "lambda -1", "refine lambda -1");
  refused(lsfa_mv_refine_chain(p, S, 1, 2, W, H, rows, 2, (1 << 24) + 1, 0, rows, nullptr, nullptr), "lambda", "refine lambda 2^24 + 1");
  refused(lsfa_mv_refine_chain(p, S, 1, 2, W, H, rows, 2, 4, -1, rows, nullptr, nullptr), "max_sad -1", "refine max_sad -1");
  refused(lsfa_mv_refine_chain(p, S, 0, 2, W, H, rows, 2, 4, 0, rows, nullptr, nullptr), "at least 1", "refine 0 chains");
  refused(lsfa_mv_refine_chain(p, S, 1, 0, W, H, rows, 2, 4, 0, rows, nullptr, nullptr), "at least 1", "refine 0 frames");
  refused(lsfa_mv_refine_chain(p, S - 4, 1, 2, W, H, rows, 2, 4, 0, rows, nullptr, nullptr), "plane stride", "refine short stride");
  refused(lsfa_mv_refine_chain(p, S + 2, 1, 2, W, H, rows, 2, 4, 0, rows, nullptr, nullptr), "multiple of 4", "refine stride + 2");
  refused(lsfa_mv_refine_chain(p, -S + 4, 1, 1, W, H, rows, 2, 4, 0, rows, nullptr, nullptr), "plane stride", "refine short negative stride");
  refused(lsfa_mv_refine_chain(p, INT64_MIN, 1, 1, W, H, rows, 2, 4, 0, rows, nullptr, nullptr), "plane stride", "refine stride INT64_MIN");
  refused(lsfa_mv_refine_chain(p + 1, S, 1, 2, W, H, rows, 2, 4, 0, rows, nullptr, nullptr), "4-byte aligned", "refine luma misaligned");
  refused(lsfa_mv_refine_chain(p, S, 1 << 14, 1 << 14, W, H, rows, 2, 4, 0, rows, nullptr, nullptr), "exceed one grid", "refine 2^28 pairs");
  refused(lsfa_mv_refine_chain(p, S, 46341, 46341, W, H, rows, 2, 4, 0, rows, nullptr, nullptr), "exceed one grid", "refine pairs beyond int");
  refused(lsfa_mv_refine_chain(p, 1LL << 32, 1 << 10, 1 << 10, 30000, 30000, rows, 2, 4, 0, rows, nullptr, nullptr), "exceed one grid", "refine 2^20 pairs of 3.5 M blocks");
  // lsfa_mv_estimate
  refused(lsfa_mv_estimate(nullptr, p, W, H, 16, 4, 0, rows, nullptr, nullptr), "NULL", "estimate cur NULL");
  refused(lsfa_mv_estimate(p, nullptr, W, H, 16, 4, 0, rows, nullptr, nullptr), "NULL", "estimate ref NULL");
  refused(lsfa_mv_estimate(p, p, W, H, 16, 4, 0, nullptr, nullptr, nullptr), "NULL", "estimate mvs NULL");
  refused(lsfa_mv_estimate(p, p, 0, H, 16, 4, 0, rows, nullptr, nullptr), "bad frame size", "estimate width 0");
  refused(lsfa_mv_estimate(p, p, W, -1, 16, 4, 0, rows, nullptr, nullptr), "bad frame size", "estimate height -1");
  refused(lsfa_mv_estimate(p, p, 1 << 16, 1 << 16, 16, 4, 0, rows, nullptr, nullptr), "bad frame size", "estimate 2^32 pixels");
  refused(lsfa_mv_estimate(p, p, W, H, 0, 4, 0, rows, nullptr, nullptr), "search 0", "estimate search 0");
  refused(lsfa_mv_estimate(p, p, W, H, 33, 4, 0, rows, nullptr, nullptr), "search 33", "estimate search 33");
  refused(lsfa_mv_estimate(p, p, W, H, 16, -1, 0, rows, nullptr, nullptr), "lambda -1", "estimate lambda -1");
  refused(lsfa_mv_estimate(p, p, W, H, 16, (1 << 24) + 1, 0, rows, nullptr, nullptr), "lambda", "estimate lambda 2^24 + 1");
  refused(lsfa_mv_estimate(p, p, W, H, 16, 4, -1, rows, nullptr, nullptr), "max_sad -1", "estimate max_sad -1");
  refused(lsfa_mv_estimate(p + 1, p, W, H, 16, 4, 0, rows, nullptr, nullptr), "4-byte aligned", "estimate cur misaligned");
  refused(lsfa_mv_estimate(p, p + 2, W, H, 16, 4, 0, rows, nullptr, nullptr), "4-byte aligned", "estimate ref misaligned");
  // lsfa_mv_estimate_chain
  refused(lsfa_mv_estimate_chain(nullptr, S, 1, 2, W, H, 16, 4, 0, rows, nullptr, nullptr), "NULL", "chain luma NULL");
  refused(lsfa_mv_estimate_chain(p, S, 1, 2, W, H, 16, 4, 0, nullptr, nullptr, nullptr), "NULL", "chain mvs NULL");
  refused(lsfa_mv_estimate_chain(p, S, 1, 2, 0, H, 16, 4, 0, rows, nullptr, nullptr), "bad frame size", "chain width 0");
  refused(lsfa_mv_estimate_chain(p, S, 1, 2, W, -1, 16, 4, 0, rows, nullptr, nullptr), "bad frame size", "chain height -1");
  refused(lsfa_mv_estimate_chain(p, S, 1, 2, W, H, 0, 4, 0, rows, nullptr, nullptr), "search 0", "chain search 0");
  refused(lsfa_mv_estimate_chain(p, S, 1, 2, W, H, 33, 4, 0, rows, nullptr, nullptr), "search 33", "chain search 33");
  refused(lsfa_mv_estimate_chain(p, S, 1, 2, W, H, 16, -1, 0, rows, nullptr, nullptr), "lambda -1", "chain lambda -1");
  refused(lsfa_mv_estimate_chain(p, S, 1, 2, W, H, 16, (1 << 24) + 1, 0, rows, nullptr, nullptr), "lambda", "chain lambda 2^24 + 1");
  refused(lsfa_mv_estimate_chain(p, S, 1, 2, W, H, 16, 4, -1, rows, nullptr, nullptr), "max_sad -1", "chain max_sad -1");
  refused(lsfa_mv_estimate_chain(p, S, 0, 2, W, H, 16, 4, 0, rows, nullptr, nullptr), "at least 1", "chain 0 chains");
  refused(lsfa_mv_estimate_chain(p, S, 1, 0, W, H, 16, 4, 0, rows, nullptr, nullptr), "at least 1", "chain 0 frames");
  refused(lsfa_mv_estimate_chain(p, S - 4, 1, 2, W, H, 16, 4, 0, rows, nullptr, nullptr), "plane stride", "chain short stride");
  refused(lsfa_mv_estimate_chain(p, S + 2, 1, 2, W, H, 16, 4, 0, rows, nullptr, nullptr), "multiple of 4", "chain stride + 2");
  refused(lsfa_mv_estimate_chain(p, -S + 4, 1, 1, W, H, 16, 4, 0, rows, nullptr, nullptr), "plane stride", "chain short negative stride");
  refused(lsfa_mv_estimate_chain(p, INT64_MIN, 1, 1, W, H, 16, 4, 0, rows, nullptr, nullptr), "plane stride", "chain stride INT64_MIN");
  refused(lsfa_mv_estimate_chain(p + 1, S, 1, 2, W, H, 16, 4, 0, rows, nullptr, nullptr), "4-byte aligned", "chain luma misaligned");
  refused(lsfa_mv_estimate_chain(p, S, 1 << 16, 1 << 12, W, H, 16, 4, 0, rows, nullptr, nullptr), "exceed one grid", "chain 2^28 pairs");
  refused(lsfa_mv_estimate_chain(p, S, 46341, 46341, W, H, 16, 4, 0, rows, nullptr, nullptr), "exceed one grid", "chain pairs beyond int");
  printf("%d of %d refusals as declared\n", checks - failures, checks);
  return failures ? 1 : 0;
}
