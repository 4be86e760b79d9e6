/* glm/glm.hpp -- stand-in for the part of glm that the reference's kernel headers use (Common/Math.h, Ray.cuh,
 * Random.cuh, ThinLensCamera.cuh, Kernels.cuh, DeviceUtils.cuh).  glm itself is not available to this build.
 *
 * TEST INFRASTRUCTURE (see oracle/ref_driver.cpp).  Written from glm's documented definitions (glm 0.9.9 manual and
 * API reference; the GLSL specification for the functions glm takes from it), NOT from the oracle's restatement: the
 * point of the compiled reference is to be a second reading.  Every function is the scalar (non-SIMD) form, which is
 * what GLM_FORCE_XYZW_ONLY (Common/Math.h:8) and a CUDA compile select.  Comments marked ORDER fix a rounding order that
 * the result's bits depend on; an ORDER choice that could not be settled from the documentation is listed in DESIGN.md.
 *
 * glm::sin, glm::cos and glm::tan go through function pointers (ref_shim::sin_fn ...), libm by default, so that the
 * driver can put the project's build-owned sincos behind them: a CUDA build would call libdevice
 * there, which no host has.
 */
#pragma once

#include <cmath>
#include <cstdint>

namespace ref_shim {
extern float (*sin_fn)(float);
extern float (*cos_fn)(float);
extern float (*tan_fn)(float);
}  // namespace ref_shim

namespace glm {

/* ---- vectors: aggregates of x, y (, z, w); a default-constructed one is zero (glm leaves it unset) ------------------ */
struct vec2 {
  float x, y;
  vec2() : x(0.0f), y(0.0f) {}
  vec2(float a, float b) : x(a), y(b) {}
  float& operator[](int i) { return i == 0 ? x : y; }
  const float& operator[](int i) const { return i == 0 ? x : y; }
  vec2& operator+=(const vec2& o) {
    x += o.x;
    y += o.y;
    return *this;
  }
};

struct uvec2 {
  uint32_t x, y;
  uvec2() : x(0), y(0) {}
  uvec2(uint32_t a, uint32_t b) : x(a), y(b) {}
};

struct ivec2 {
  int32_t x, y;
  ivec2() : x(0), y(0) {}
  ivec2(int32_t a, int32_t b) : x(a), y(b) {}
};

struct uvec3 {
  uint32_t x, y, z;
  uvec3() : x(0), y(0), z(0) {}
  uvec3(uint32_t a, uint32_t b, uint32_t c) : x(a), y(b), z(c) {}
};

struct vec4;

struct vec3 {
  float x, y, z;
  vec3() : x(0.0f), y(0.0f), z(0.0f) {}
  explicit vec3(float s) : x(s), y(s), z(s) {}
  vec3(float a, float b, float c) : x(a), y(b), z(c) {}
  vec3(const vec2& v, float c) : x(v.x), y(v.y), z(c) {}
  explicit vec3(const vec4& v); /* drops w */
  float& operator[](int i) { return (&x)[i]; }
  const float& operator[](int i) const { return (&x)[i]; }
  vec3& operator+=(const vec3& o) {
    x += o.x;
    y += o.y;
    z += o.z;
    return *this;
  }
};

struct vec4 {
  float x, y, z, w;
  vec4() : x(0.0f), y(0.0f), z(0.0f), w(0.0f) {}
  explicit vec4(float s) : x(s), y(s), z(s), w(s) {}
  vec4(float a, float b, float c, float d) : x(a), y(b), z(c), w(d) {}
  vec4(const vec3& v, float d) : x(v.x), y(v.y), z(v.z), w(d) {}
  float& operator[](int i) { return (&x)[i]; }
  const float& operator[](int i) const { return (&x)[i]; }
};

inline vec3::vec3(const vec4& v) : x(v.x), y(v.y), z(v.z) {}

/* component-wise operators; vector * scalar and scalar * vector multiply each component once */
inline vec2 operator*(const vec2& v, float s) { return vec2(v.x * s, v.y * s); }
inline vec3 operator+(const vec3& a, const vec3& b) { return vec3(a.x + b.x, a.y + b.y, a.z + b.z); }
inline vec3 operator-(const vec3& a, const vec3& b) { return vec3(a.x - b.x, a.y - b.y, a.z - b.z); }
inline vec3 operator*(const vec3& a, const vec3& b) { return vec3(a.x * b.x, a.y * b.y, a.z * b.z); }
inline vec3 operator*(const vec3& v, float s) { return vec3(v.x * s, v.y * s, v.z * s); }
inline vec3 operator*(float s, const vec3& v) { return vec3(s * v.x, s * v.y, s * v.z); }
inline vec4 operator+(const vec4& a, const vec4& b) { return vec4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
inline vec4 operator*(const vec4& v, float s) { return vec4(v.x * s, v.y * s, v.z * s, v.w * s); }

/* ---- geometric functions ------------------------------------------------------------------------------------------ */
/* ORDER: glm's dot of two vec3 multiplies component-wise into a temporary and returns tmp.x + tmp.y + tmp.z, which C++
 * evaluates as (x + y) + z. */
inline float dot(const vec3& a, const vec3& b) {
  const vec3 tmp(a * b);
  return tmp.x + tmp.y + tmp.z;
}

/* ORDER: glm's cross is (x.y*y.z - y.y*x.z, x.z*y.x - y.z*x.x, x.x*y.y - y.x*x.y): the first product holds the left
 * operand's earlier-cycled component.  (Each component is a difference of two rounded products; which product is written
 * first does not change the bits, the pairing does.) */
inline vec3 cross(const vec3& x, const vec3& y) {
  return vec3(x.y * y.z - y.y * x.z, x.z * y.x - y.z * x.x, x.x * y.y - y.x * x.y);
}

/* ORDER: glm's inversesqrt(x) is 1 / sqrt(x) (correctly rounded sqrt, then a correctly rounded division), and
 * normalize(v) is v * inversesqrt(dot(v, v)): one reciprocal, three products -- not three divisions by the length. */
inline float inversesqrt(float x) { return 1.0f / std::sqrt(x); }
inline vec3 normalize(const vec3& v) { return v * inversesqrt(dot(v, v)); }

inline vec3 abs(const vec3& v) { return vec3(std::fabs(v.x), std::fabs(v.y), std::fabs(v.z)); }

/* ---- angles and trigonometry --------------------------------------------------------------------------------------- */
/* ORDER: glm's radians is degrees * 0.01745329251994329576923690768489 in the argument's type: one fp32 product with
 * the fp32 nearest to pi / 180 (not degrees * pi / 180 in two steps). */
inline float radians(float degrees) { return degrees * 0.01745329251994329576923690768489f; }
inline float sin(float x) { return ref_shim::sin_fn(x); }
inline float cos(float x) { return ref_shim::cos_fn(x); }
inline float tan(float x) { return ref_shim::tan_fn(x); }
inline float ceil(float x) { return std::ceil(x); }

/* ---- mat4: four column vectors ------------------------------------------------------------------------------------- */
struct mat4 {
  vec4 col[4];
  mat4() { /* glm leaves it unset; identity here */
    col[0] = vec4(1, 0, 0, 0);
    col[1] = vec4(0, 1, 0, 0);
    col[2] = vec4(0, 0, 1, 0);
    col[3] = vec4(0, 0, 0, 1);
  }
  vec4& operator[](int i) { return col[i]; }
  const vec4& operator[](int i) const { return col[i]; }
};

/* ORDER: glm's mat4 * vec4 is the sum of the columns scaled by the vector's components, paired as
 * (m[0]*v.x + m[1]*v.y) + (m[2]*v.z + m[3]*v.w) -- Mul0 + Mul1 = Add0, Mul2 + Mul3 = Add1, Add0 + Add1 -- and not a
 * left-to-right sum of the four products nor a dot product per row. */
inline vec4 operator*(const mat4& m, const vec4& v) {
  const vec4 add0 = m[0] * v.x + m[1] * v.y;
  const vec4 add1 = m[2] * v.z + m[3] * v.w;
  return add0 + add1;
}

/* ---- quat (glm/gtx/quaternion.hpp includes this file; the quaternion lives here so that Common/Math.h's aliases see
 *      it whichever header comes first) ------------------------------------------------------------------------------ */
struct quat {
  float x, y, z, w;
  quat() : x(0.0f), y(0.0f), z(0.0f), w(1.0f) {}
  quat(float w_, float x_, float y_, float z_) : x(x_), y(y_), z(z_), w(w_) {} /* glm's argument order: w first */
};

/* ORDER: glm's Hamilton product p * q, each component a left-to-right chain of four products:
 *   w = p.w*q.w - p.x*q.x - p.y*q.y - p.z*q.z
 *   x = p.w*q.x + p.x*q.w + p.y*q.z - p.z*q.y
 *   y = p.w*q.y + p.y*q.w + p.z*q.x - p.x*q.z
 *   z = p.w*q.z + p.z*q.w + p.x*q.y - p.y*q.x */
inline quat operator*(const quat& p, const quat& q) {
  return quat(p.w * q.w - p.x * q.x - p.y * q.y - p.z * q.z,
              p.w * q.x + p.x * q.w + p.y * q.z - p.z * q.y,
              p.w * q.y + p.y * q.w + p.z * q.x - p.x * q.z,
              p.w * q.z + p.z * q.w + p.x * q.y - p.y * q.x);
}

/* ORDER: glm's angleAxis(angle, axis) is quat(cos(angle * 0.5), axis * sin(angle * 0.5)): the half angle is one product
 * with 0.5f (exact), sin and cos are taken of that, and the axis is not normalised. */
inline quat angleAxis(float angle, const vec3& axis) {
  const float s = glm::sin(angle * 0.5f);
  return quat(glm::cos(angle * 0.5f), axis.x * s, axis.y * s, axis.z * s);
}

/* ORDER: glm's mat3_cast, which mat4_cast wraps into a mat4 with a (0, 0, 0, 1) last row and column.  Nine products
 * qxx = q.x*q.x ... qwz = q.w*q.z, then per entry  1 - 2*(a + b)  on the diagonal and  2*(a + b) / 2*(a - b)  off it:
 *   [0] = (1 - 2(qyy + qzz),     2(qxy + qwz),     2(qxz - qwy))
 *   [1] = (    2(qxy - qwz), 1 - 2(qxx + qzz),     2(qyz + qwx))
 *   [2] = (    2(qxz + qwy),     2(qyz - qwx), 1 - 2(qxx + qyy))     ([c] is column c) */
inline mat4 mat4_cast(const quat& q) {
  const float qxx = q.x * q.x, qyy = q.y * q.y, qzz = q.z * q.z;
  const float qxz = q.x * q.z, qxy = q.x * q.y, qyz = q.y * q.z;
  const float qwx = q.w * q.x, qwy = q.w * q.y, qwz = q.w * q.z;
  mat4 r;
  r[0] = vec4(1.0f - 2.0f * (qyy + qzz), 2.0f * (qxy + qwz), 2.0f * (qxz - qwy), 0.0f);
  r[1] = vec4(2.0f * (qxy - qwz), 1.0f - 2.0f * (qxx + qzz), 2.0f * (qyz + qwx), 0.0f);
  r[2] = vec4(2.0f * (qxz + qwy), 2.0f * (qyz - qwx), 1.0f - 2.0f * (qxx + qyy), 0.0f);
  r[3] = vec4(0.0f, 0.0f, 0.0f, 1.0f);
  return r;
}

}  // namespace glm
