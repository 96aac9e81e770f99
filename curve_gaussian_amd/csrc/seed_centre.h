// The lattice that the edge vote (edge_seed.hip) and the distance field (tsdf.hip) share: the centres of a SeedGrid's voxels.
#pragma once
#include "kernels.h"

namespace cgs {

// The centre of the voxel with linear index `id` (x fastest): float64, then the float32 point that the projection contract
// is written for, widened again.
__device__ inline void seed_centre(const SeedGrid& g, long long id, double& X, double& Y, double& Z) {
#pragma clang fp contract(off)
    const int i = (int)(id % g.nx);
    const long long r = id / g.nx;
    const int j = (int)(r % g.ny), k = (int)(r / g.ny);
    X = (double)(float)(g.lo[0] + ((double)i + 0.5) * g.step[0]);
    Y = (double)(float)(g.lo[1] + ((double)j + 0.5) * g.step[1]);
    Z = (double)(float)(g.lo[2] + ((double)k + 0.5) * g.step[2]);
}

}  // namespace cgs
