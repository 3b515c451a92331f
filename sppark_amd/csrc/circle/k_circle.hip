// Explicit instantiation of the circle transform's pass kernel (circle_kernels.hpp) for one direction
// (-DSPPARK_CIRCLE_INV=0: evaluate, =1: interpolate); Mersenne31 only.
#include "circle_kernels.hpp"
#ifndef SPPARK_CIRCLE_INV
# error "compile with -DSPPARK_CIRCLE_INV=0 or 1"
#endif
#ifndef FEATURE_MERSENNE31
# error "the circle transform is defined over Mersenne31 only"
#endif
namespace sppark_amd {
template __global__ void k_circle_pass<(SPPARK_CIRCLE_INV != 0)>(cf_t*, size_t, size_t, circle_pass, const circle_pt*);
}
