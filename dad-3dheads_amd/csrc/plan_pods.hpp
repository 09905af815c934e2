// Plain twins of HIP's vector types for the host planners (flame_plan.hpp, mesh_plan.hpp), which compile without the HIP headers. Same
// members, same size; capi_checks.hpp asserts it, and DeviceArray::upload copies a vector of them into the HIP type's array.
#pragma once

namespace dad3d {
namespace plan {

struct Int4 {
    int x, y, z, w;
};
struct UInt2 {
    unsigned x, y;
};
struct UInt4 {
    unsigned x, y, z, w;
};
struct Float4 {
    float x, y, z, w;
};

}  // namespace plan
}  // namespace dad3d
