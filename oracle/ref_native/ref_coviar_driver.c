/* Host driver of the reference's own motion-vector accumulation, create_and_load_mv_residual.
 *
 * The function is NOT in this file: the build cuts it (and the two #defines it reads) out of the reference's
 * coviar_data_loader.c into _ref/coviar.inc, which is never committed.  Here are stand-ins for the three
 * types it touches, with only the members it reads, and the frame loop of decode_video that feeds it.
 */
#include <assert.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

/* libavutil/motion_vector.h's block record, in its field order and widths */
typedef struct AVMotionVector {
  int32_t source;
  uint8_t w, h;
  int16_t src_x, src_y;
  int16_t dst_x, dst_y;
  uint64_t flags;
} AVMotionVector;

typedef struct AVFrameSideData {
  uint8_t* data;
  int size;
} AVFrameSideData;

/* a C-contiguous 3-D array, as PyArray_ZEROS makes it */
typedef struct PyArrayObject {
  char* data;
  long strides[3];
} PyArrayObject;
#define PyArray_GETPTR3(a, i, j, k) \
  ((void*)((a)->data + (long)(i) * (a)->strides[0] + (long)(j) * (a)->strides[1] + (long)(k) * (a)->strides[2]))

#include "coviar.inc"

static void wrap(PyArrayObject* a, void* data, int d1, int d2, int item) {
  a->data = (char*)data;
  a->strides[2] = item;
  a->strides[1] = (long)d2 * item;
  a->strides[0] = (long)d1 * d2 * item;
}

/* One GOP, accumulate = 1, as decode_video drives it (coviar_data_loader.c:316-360): both maps start as the
 * identity in the reference's x-major layout, frame f of `frames` is cur_pos = f + 1 (cur_pos 0 is the I-frame,
 * which carries no vectors), the target is the last frame.  A frame without rows is passed as an empty side-data
 * block.  rows (sum of counts, 7) int32 {source, w, h, src_x, src_y, dst_x, dst_y}; the caller keeps them
 * within AVMotionVector's field widths.  representation: 1 = MV, 2 = RESIDUAL, the loader's two modes.
 * accu_after (frames, width, height, 2) receives the x-major map after every frame; mv (height, width, 2)
 * and res (height, width, 3) are what the loader returns; bgr (2, height, width, 3) = {reference frame, target frame}.
 * Returns 0, or -1 for a row outside the field widths. */
int ref_coviar_gop(const int32_t* rows, const int* counts, int frames, int width, int height, int representation,
                   uint8_t* bgr, int32_t* accu_after, int32_t* mv, int32_t* res) {
  const size_t map = (size_t)width * height * 2;
  int* accu_src = (int*)malloc(map * sizeof(int));
  int* accu_src_old = (int*)malloc(map * sizeof(int));
  for (size_t p = 0; p < (size_t)width * height; ++p) {      /* x-major: pixel (x, y) at p = x * height + y */
    accu_src_old[p * 2] = (int)(p / height);
    accu_src_old[p * 2 + 1] = (int)(p % height);
  }
  memcpy(accu_src, accu_src_old, map * sizeof(int));
  PyArrayObject bgr_arr, mv_arr, res_arr;
  wrap(&bgr_arr, bgr, height * width, 3, 1);
  wrap(&mv_arr, mv, width, 2, 4);
  wrap(&res_arr, res, width, 3, 4);
  int status = 0;
  for (int f = 0; f < frames && status == 0; ++f) {
    const int n = counts[f];
    AVMotionVector* blocks = (AVMotionVector*)calloc((size_t)(n > 0 ? n : 1), sizeof(AVMotionVector));
    for (int i = 0; i < n; ++i) {
      const int32_t* r = rows + (size_t)i * 7;
      if (r[1] < 0 || r[1] > 255 || r[2] < 0 || r[2] > 255) status = -1;
      for (int k = 3; k < 7; ++k)
        if (r[k] < -32768 || r[k] > 32767) status = -1;
      blocks[i].source = r[0];
      blocks[i].w = (uint8_t)r[1]; blocks[i].h = (uint8_t)r[2];
      blocks[i].src_x = (int16_t)r[3]; blocks[i].src_y = (int16_t)r[4];
      blocks[i].dst_x = (int16_t)r[5]; blocks[i].dst_y = (int16_t)r[6];
    }
    rows += (size_t)n * 7;
    if (status == 0) {
      AVFrameSideData sd;
      sd.data = (uint8_t*)blocks;
      sd.size = (int)(n * sizeof(AVMotionVector));
      create_and_load_mv_residual(&sd, &bgr_arr, &mv_arr, &res_arr, f + 1, 1, representation, accu_src, accu_src_old,
                                  width, height, frames);
      memcpy(accu_after + (size_t)f * map, accu_src, map * sizeof(int));
    }
    free(blocks);
  }
  free(accu_src_old), free(accu_src);
  return status;
}
