// Host interface of the streamed attention family (attention_stream.hip): the kernels that take the sequence
// lengths the LDS-resident kernels of attention.hip refuse.  attention.hip owns the dispatch rule and the plan
// string; this header only carries the launchers and the sizes they use.
#pragma once

#include "common.h"

// queries per workgroup (forward, backward dQ), keys per workgroup (backward dK / dV), keys or queries per LDS chunk
struct MhaStreamSizes { int q, k, c; };
MhaStreamSizes mha_stream_sizes(int dtype, int backward);

int mha_stream_fwd(const void* qkv, void* out, float* lse, int B, int T, int H, int dh, float scale, int dtype,
                   hipStream_t st);
int mha_stream_bwd(const void* qkv, const void* o, const void* dout, const float* lse, void* dqkv, int B, int T, int H,
                   int dh, float scale, int dtype, hipStream_t st);
