// Squared distance of two points, shared by the point-set kernels (knn.hip, radius.hip, fps.hip).
#pragma once

// fp64 dx*dx + dy*dy (+ dz*dz), each operation rounded on its own (no FMA contraction): the
// arithmetic of the float64 restatements, so selections made from it are bit-exact against them.
// Plain operators in a contract(off) scope: HIP's __dmul_rn / __dadd_rn carry their header's
// `contract` flag and still fuse into an FMA under the default -ffp-contract=fast.
__device__ __forceinline__ double sqd(const double* a, const double* b, int D) {
#pragma clang fp contract(off)
  const double dx = a[0] - b[0], dy = a[1] - b[1];
  double s = dx * dx + dy * dy;
  if (D == 3) {
    const double dz = a[2] - b[2];
    s = s + dz * dz;
  }
  return s;
}
