/* cuda_runtime.h -- stand-in, so that the reference's kernel headers compile as host C++.
 *
 * TEST INFRASTRUCTURE (see oracle/ref_driver.cpp): the reference's RayTracer/Kernels.cuh and what it includes are
 * compiled unmodified against the headers of this folder, and its __global__ functions are then called as plain
 * functions, one call per thread of the grid.  Nothing here is taken from the CUDA toolkit: the names are the ones the
 * reference's text uses, their meaning is the documented one (CUDA C++ Programming Guide: built-in variables, vector
 * types, texture fetches).
 */
#pragma once

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>

/* function space qualifiers mean nothing to a host compile */
#define __device__
#define __host__
#define __global__

struct float4 {
  float x, y, z, w;
};

struct dim3 {
  unsigned int x, y, z;
};

/* The built-in variables of a kernel: the driver sets them before each call of a __global__ function.  Thread-local, so
 * that several host threads could each play a CUDA thread. */
extern thread_local dim3 blockIdx, blockDim, threadIdx;

/* A texture object is a pointer to its float4 texels; the texture is one row of ref_shim::tex_width texels (the
 * reference's scene texture is one row: RayTracerImpl.cu:151-157). */
typedef const float4* cudaTextureObject_t;

namespace ref_shim {
extern thread_local unsigned int tex_width;
}

/* tex2D with the reference's texture settings (RayTracerImpl.cu:169-173: clamp addressing, point filtering, element
 * read mode, and normalizedCoords left 0): texel floor(x) of the row, x clamped to the row; y addresses the only row. */
template <class T>
inline T tex2D(cudaTextureObject_t tex, float x, float /*y*/) {
  long i = static_cast<long>(std::floor(x));
  const long last = static_cast<long>(ref_shim::tex_width) - 1;
  i = i < 0 ? 0 : (i > last ? last : i);
  return tex[i];
}
