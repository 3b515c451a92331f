// C-ABI of a polynomial-primitives-only library (-DFEATURE_MERSENNE31 / -DFEATURE_BABY_BEAR_X4):
// fields the reference defines as types only (ff/mersenne31.hpp, bb31_4_t in ff/baby_bear.hpp) with
// no NTT parameter set; the generic primitives of polynomial/*.cuh are their natural entry points.
#include "../ntt/field_select.hpp"
#include "common_api.hpp"

using namespace sppark_amd;
typedef ntt_fr_t fr_t;

#include "poly_api.hpp"
#include "field_api.hpp"
#include "vec_api.hpp"
#include "mle_api.hpp"
#include "merkle_api.hpp"
#include "fri_api.hpp"
