// Stand-in for rmagine's EmbreeMap: a handle to the ORACLE'S scene (oracle/radarays_oracle.h) plus the per-face object
// ids, so that the reference loop and the oracle query the very same nearest-hit function.  TEST INFRASTRUCTURE ONLY.
#pragma once
#include <memory>
#include <stdint.h>

struct orc_scene;

namespace rmagine {

struct EmbreeMap {
    const orc_scene* scene = nullptr;
    const uint32_t* face_object_id = nullptr;   // [n_faces] or null (every face is object 0)
};

using EmbreeMapPtr = std::shared_ptr<EmbreeMap>;

}  // namespace rmagine
