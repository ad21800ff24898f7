// Behaving stand-in for rmagine's OnDnSimulatorEmbree -- TEST INFRASTRUCTURE ONLY.
// The ray cast as DESIGN.md §2 item 1 states it: o_w = Tsm Tsb o, d_w = R d, tnear = 0, tfar = range.max; the result
// is the range, the geometric face normal (normalised, rotated into the sensor frame, flipped against the ray) and the
// object id, UINT_MAX on a miss.  The nearest hit itself is the oracle's orc_intersect: one function on both sides.
#pragma once
#include <limits.h>
#include <memory>

#include <rmagine/map/EmbreeMap.hpp>
#include <rmagine/math/types.h>
#include <rmagine/types/Memory.hpp>
#include <rmagine/types/sensor_models.h>

extern "C" int orc_intersect(const orc_scene*, const float orig[3], const float dir[3],
                             float* t, uint32_t* tri, float ng[3]);

namespace rmagine {

template <typename MemT> struct Hits { Memory<uint8_t, MemT> hits; };
template <typename MemT> struct Ranges { Memory<float, MemT> ranges; };
template <typename MemT> struct Normals { Memory<Vector, MemT> normals; };
template <typename MemT> struct ObjectIds { Memory<unsigned int, MemT> object_ids; };

template <typename... Ts> struct Bundle : public Ts... {};

class OnDnSimulatorEmbree {
public:
    explicit OnDnSimulatorEmbree(EmbreeMapPtr map) : m_map(map) {}
    void setTsb(const Transform& Tsb) { m_Tsb = Tsb; }
    void setModel(const OnDnModel& model) { m_model = model; }

    template <typename BundleT>
    void simulate(const MemView<Transform>& Tbm, BundleT& ret) const
    {
        const size_t n = m_model.size();
        for (size_t pid = 0; pid < Tbm.size(); pid++) {
            const Transform Tsm = Tbm[pid] * m_Tsb;
            const Quaternion Rms = Tsm.R.inv();
            for (size_t i = 0; i < n; i++) {
                const size_t k = pid * n + i;
                const Vector d_s = m_model.dirs[i];
                const Vector o_w = Tsm * m_model.origs[i];
                const Vector d_w = Tsm.R * d_s;
                const float o[3] = {o_w.x, o_w.y, o_w.z}, d[3] = {d_w.x, d_w.y, d_w.z};
                float t = 0.0f, ng[3] = {0.0f, 0.0f, 0.0f};
                uint32_t face = 0;
                const bool hit = m_map && m_map->scene && orc_intersect(m_map->scene, o, d, &t, &face, ng) &&
                                 t <= m_model.range.max;
                if (hit) {
                    Vector nint = {ng[0], ng[1], ng[2]};
                    nint.normalizeInplace();
                    nint = Rms * nint;
                    if (d_s.dot(nint) > 0.0f) nint = -nint;
                    ret.hits[k] = 1;
                    ret.ranges[k] = t;
                    ret.normals[k] = nint;
                    ret.object_ids[k] = m_map->face_object_id ? m_map->face_object_id[face] : 0u;
                } else {
                    ret.hits[k] = 0;
                    ret.ranges[k] = m_model.range.max + 1.0f;
                    ret.normals[k] = Vector::Zeros();
                    ret.object_ids[k] = UINT_MAX;
                }
            }
        }
    }

private:
    EmbreeMapPtr m_map;
    Transform m_Tsb = Transform::Identity();
    OnDnModel m_model;
};

using OnDnSimulatorEmbreePtr = std::shared_ptr<OnDnSimulatorEmbree>;

}  // namespace rmagine
