// lsfa_conv_pair_fwd: a ResNet unit's conv3 + shortcut add and the next unit's conv1 in one launch (conv_pair_kernel.h;
// dff_rfcn/symbols/resnet.py:70-101).  Two fp16 pieces, per-channel weight scales, dense channels-last maps only; everything else is
// LSFA_ENOTSUP and stays on two lsfa_conv_fwd launches.  No workspace, no allocation, no synchronisation.
#include "common.h"

#include "conv_pair_kernel.h"

using namespace lsfa;

namespace {
struct PairKernel { int cm, cn; void (*fn)(convsplit::PairArgs); };
const PairKernel kPairKernels[] = {{64, 64, convsplit::conv_pair_kernel<2, 2>},
                                   {64, 128, convsplit::conv_pair_kernel<2, 4>},
                                   {128, 64, convsplit::conv_pair_kernel<4, 2>},
                                   {128, 128, convsplit::conv_pair_kernel<4, 4>}};
}  // namespace

extern "C" int lsfa_conv_pair_fwd(const float* x, int ldx, int N, int H, int W, int Cm, const float* amax_in, const void* w3frag,
                                  const float* w3_scale, int pieces3, int C, const float* residual, float* y, int ldy, const float* scale2,
                                  const float* shift2, const void* w1frag, const float* w1_scale, int pieces1, int Cn, const float* bias,
                                  float* z, int ldz, int stride, int y_nchw, unsigned* amax_out_sum, unsigned* amax_out_z, unsigned* status,
                                  void* stream) {
  const char* who = "lsfa_conv_pair_fwd";
  LSFA_REQUIRE(N > 0 && H > 0 && W > 0 && Cm > 0 && C > 0 && Cn > 0, "%s: bad shape", who);
  if (pieces3 != 2 || pieces1 != 2) {
    set_error("%s: both weights must be cut into two fp16 pieces (pieces %d / %d)", who, pieces3, pieces1);
    return LSFA_ENOTSUP;
  }
  if (C != 4 * Cm || (Cm != 64 && Cm != 128) || (Cn != 64 && Cn != 128)) {
    set_error("%s: Cm=%d and Cn=%d must be 64 or 128 and C=%d must be 4 Cm", who, Cm, Cn, C);
    return LSFA_ENOTSUP;
  }
  if (ldx != Cm || ldy != C || ldz != Cn || y_nchw || stride != 1) {
    set_error("%s: dense channels-last maps at stride 1 only (ldx %d, ldy %d, ldz %d, y_nchw %d, stride %d)", who, ldx, ldy, ldz, y_nchw, stride);
    return LSFA_ENOTSUP;
  }
  LSFA_REQUIRE(x && amax_in && w3frag && w3_scale && residual && y && scale2 && shift2 && w1frag && w1_scale && z, "%s: NULL argument", who);
  LSFA_REQUIRE((((uintptr_t)x | (uintptr_t)residual | (uintptr_t)y | (uintptr_t)z | (uintptr_t)scale2 | (uintptr_t)shift2 | (uintptr_t)bias) & 15) == 0,
               "%s: operands must be 16-byte aligned", who);
  LSFA_REQUIRE((const void*)z != (const void*)y && (const void*)z != (const void*)x && (const void*)y != (const void*)x, "%s: x, y and z must not alias", who);
  const long P = (long)N * H * W;
  LSFA_REQUIRE((P + 128) * C < (1L << 31), "%s: tensor too large", who);
  convsplit::PairArgs a = {};
  a.x = x; a.amax = amax_in;
  a.w3 = (const uint4*)w3frag; a.w3scale = w3_scale; a.res = residual; a.y = y; a.scale2 = scale2; a.shift2 = shift2;
  a.w1 = (const uint4*)w1frag; a.w1scale = w1_scale; a.bias = bias; a.z = z;
  a.amax_sum = amax_out_sum; a.amax_z = amax_out_z; a.status = status;
  a.P = (int)P;
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof(LSFA_OP_CONV, s);
  for (const PairKernel& k : kPairKernels)
    if (k.cm == Cm && k.cn == Cn) hipLaunchKernelGGL(k.fn, dim3((unsigned)((P + 127) / 128)), dim3(convsplit::kThreads), 0, s, a);
  LSFA_LAUNCH_CHECK(who);
  return LSFA_OK;
}
