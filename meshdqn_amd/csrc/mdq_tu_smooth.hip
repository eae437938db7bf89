// Translation unit: the three smoothing kernel files (mdq_smooth / mdq_smooth_fast hand meshes to each other's kernels); each
// includes mdq_smooth_shared.hip, the reductions, the block scan and the exact update they have in common.
#include "mdq_smooth_big.hip"
#include "mdq_smooth.hip"
#include "mdq_smooth_linear.hip"
