// Behaving stand-in for rmagine's math types -- TEST INFRASTRUCTURE ONLY (oracle/refshim/README.md).
// Written from DESIGN.md §2 item 1 and the public rmagine 2.2.x interface, not from any reference text: these are the
// BUILD'S statements of rmagine's conventions, held here and nowhere else.  f32 throughout, op order as stated.
#pragma once
// rmagine's own header pulls in the C header, which makes the float overloads of acos / cos / abs visible in the global
// namespace; the reference's unqualified calls resolve against them.
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

namespace rmagine {

struct Vector {
    float x, y, z;

    static Vector Zeros() { return {0.0f, 0.0f, 0.0f}; }
    Vector operator+(const Vector& b) const { return {x + b.x, y + b.y, z + b.z}; }
    Vector operator-(const Vector& b) const { return {x - b.x, y - b.y, z - b.z}; }
    Vector operator-() const { return {-x, -y, -z}; }
    // the scalar is the vector's own type: a double factor is narrowed to f32 first
    Vector operator*(const float& s) const { return {x * s, y * s, z * s}; }
    Vector operator/(const float& s) const { return {x / s, y / s, z / s}; }
    float dot(const Vector& b) const { return x * b.x + y * b.y + z * b.z; }
    Vector cross(const Vector& b) const { return {y * b.z - z * b.y, z * b.x - x * b.z, x * b.y - y * b.x}; }
    float l2normSquared() const { return x * x + y * y + z * z; }
    float l2norm() const { return sqrtf(l2normSquared()); }
    void normalizeInplace() { const float d = l2norm(); x /= d; y /= d; z /= d; }
    Vector normalize() const { Vector r = *this; r.normalizeInplace(); return r; }
    Vector normalized() const { return normalize(); }
};

struct Quaternion;
struct Matrix3x3;

// {roll, pitch, yaw}; to a quaternion in ZYX order
struct EulerAngles {
    float roll, pitch, yaw;
    inline operator Quaternion() const;
    inline Vector operator*(const Vector& v) const;
};

struct Quaternion {
    float x, y, z, w;

    static Quaternion Identity() { return {0.0f, 0.0f, 0.0f, 1.0f}; }
    Quaternion inv() const { return {-x, -y, -z, w}; }
    // Hamilton product
    Quaternion mult(const Quaternion& b) const
    {
        Quaternion r;
        r.x = w * b.x + x * b.w + y * b.z - z * b.y;
        r.y = w * b.y - x * b.z + y * b.w + z * b.x;
        r.z = w * b.z + x * b.y - y * b.x + z * b.w;
        r.w = w * b.w - x * b.x - y * b.y - z * b.z;
        return r;
    }
    // q * v = (q (v, 0) q^-1).xyz
    Vector mult(const Vector& v) const
    {
        const Quaternion p = {v.x, v.y, v.z, 0.0f};
        const Quaternion pt = mult(p).mult(inv());
        return {pt.x, pt.y, pt.z};
    }
    Quaternion operator*(const Quaternion& b) const { return mult(b); }
    Vector operator*(const Vector& v) const { return mult(v); }
};

inline EulerAngles::operator Quaternion() const
{
    const float cr = cosf(roll / 2.0f), sr = sinf(roll / 2.0f);
    const float cp = cosf(pitch / 2.0f), sp = sinf(pitch / 2.0f);
    const float cy = cosf(yaw / 2.0f), sy = sinf(yaw / 2.0f);
    Quaternion q;
    q.w = cr * cp * cy + sr * sp * sy;
    q.x = sr * cp * cy - cr * sp * sy;
    q.y = cr * sp * cy + sr * cp * sy;
    q.z = cr * cp * sy - sr * sp * cy;
    return q;
}

inline Vector EulerAngles::operator*(const Vector& v) const
{
    const Quaternion q = *this;
    return q * v;
}

// column access (row, col); only the conversion to a quaternion is used by the sources this stands in for, and only
// outside the per-azimuth loop
struct Matrix3x3 {
    float m[3][3];
    float& operator()(unsigned r, unsigned c) { return m[r][c]; }
    const float& operator()(unsigned r, unsigned c) const { return m[r][c]; }
    operator Quaternion() const
    {
        Quaternion q;
        const float tr = m[0][0] + m[1][1] + m[2][2];
        if (tr > 0.0f) {
            const float s = sqrtf(tr + 1.0f) * 2.0f;
            q.w = 0.25f * s; q.x = (m[2][1] - m[1][2]) / s; q.y = (m[0][2] - m[2][0]) / s; q.z = (m[1][0] - m[0][1]) / s;
        } else if (m[0][0] > m[1][1] && m[0][0] > m[2][2]) {
            const float s = sqrtf(1.0f + m[0][0] - m[1][1] - m[2][2]) * 2.0f;
            q.w = (m[2][1] - m[1][2]) / s; q.x = 0.25f * s; q.y = (m[0][1] + m[1][0]) / s; q.z = (m[0][2] + m[2][0]) / s;
        } else if (m[1][1] > m[2][2]) {
            const float s = sqrtf(1.0f + m[1][1] - m[0][0] - m[2][2]) * 2.0f;
            q.w = (m[0][2] - m[2][0]) / s; q.x = (m[0][1] + m[1][0]) / s; q.y = 0.25f * s; q.z = (m[1][2] + m[2][1]) / s;
        } else {
            const float s = sqrtf(1.0f + m[2][2] - m[0][0] - m[1][1]) * 2.0f;
            q.w = (m[1][0] - m[0][1]) / s; q.x = (m[0][2] + m[2][0]) / s; q.y = (m[1][2] + m[2][1]) / s; q.z = 0.25f * s;
        }
        return q;
    }
};

// a Quaternion member that can be assigned Euler angles or a matrix, as rmagine's can
struct Rotation : Quaternion {
    Rotation() = default;
    Rotation(const Quaternion& q) : Quaternion(q) {}
    Rotation& operator=(const Quaternion& q) { Quaternion::operator=(q); return *this; }
    Rotation& operator=(const EulerAngles& e) { Quaternion::operator=(static_cast<Quaternion>(e)); return *this; }
    Rotation& operator=(const Matrix3x3& M) { Quaternion::operator=(static_cast<Quaternion>(M)); return *this; }
};

// T1 * T2 = {R1 R2, R1 t2 + t1}
struct Transform {
    Rotation R;
    Vector t;

    static Transform Identity()
    {
        Transform T;
        T.R = Quaternion::Identity();
        T.t = Vector::Zeros();
        return T;
    }
    Transform inv() const
    {
        Transform T;
        T.R = R.inv();
        T.t = -(T.R * t);
        return T;
    }
    Transform mult(const Transform& b) const
    {
        Transform T;
        T.R = R * b.R;
        T.t = R * b.t + t;
        return T;
    }
    Transform operator*(const Transform& b) const { return mult(b); }
    Vector operator*(const Vector& v) const { return R * v + t; }
};

}  // namespace rmagine
