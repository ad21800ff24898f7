// Behaving stand-in for rmagine's sensor models -- TEST INFRASTRUCTURE ONLY.
#pragma once
#include <rmagine/math/types.h>
#include <rmagine/types/Memory.hpp>

namespace rmagine {

struct Interval { float min, max; };

struct DiscreteInterval {
    float min, inc;
    uint32_t size;
    float getValue(uint32_t id) const { return min + static_cast<float>(id) * inc; }
};

// getTheta(h) = theta.min + h * theta.inc; every ray starts at the sensor's origin
struct SphericalModel {
    DiscreteInterval phi, theta;
    Interval range;
    uint32_t getWidth() const { return theta.size; }
    uint32_t getHeight() const { return phi.size; }
    float getPhi(uint32_t vid) const { return phi.getValue(vid); }
    float getTheta(uint32_t hid) const { return theta.getValue(hid); }
    Vector getOrigin(uint32_t, uint32_t) const { return Vector::Zeros(); }
};

// one origin and one direction per ray, in the sensor frame
struct OnDnModel {
    uint32_t width = 0, height = 0;
    Interval range = {0.0f, 0.0f};
    Memory<Vector, RAM> origs, dirs;
    uint32_t getWidth() const { return width; }
    uint32_t getHeight() const { return height; }
    uint32_t size() const { return width * height; }
    uint32_t getBufferId(uint32_t vid, uint32_t hid) const { return vid * width + hid; }
    Vector getOrigin(uint32_t vid, uint32_t hid) const { return origs[getBufferId(vid, hid)]; }
    Vector getDirection(uint32_t vid, uint32_t hid) const { return dirs[getBufferId(vid, hid)]; }
};

}  // namespace rmagine
