// eigen3 of lib/utilities/utilities.f90:107-201 restated as it is written, for every kernel that needs the principal values of a
// symmetric 3 x 3 tensor: the Mohr-Coulomb return mapping (fx_yield.h) and the principal stresses and strains of the nodal output
// (fx_nodal_stress.h).  The reference's `stop` sets the kernels' error word (FX_YERR_JACOBI); the host entry point then returns
// FX_ERROR_RUNTIME with the reference's text.
//
// Two instantiations of one text (fx_eigen3_body.h): yield_eigen3 leaves the contraction of products and sums to the compiler, as the
// material point always has (its results do not change); exact_eigen3 keeps them apart, as the reference's compilers do, so that the
// principal values of the output agree with the reference to the last bit.
//
// Registers: the three rotations are instantiated for their compile-time (ip, iq) -- no array is indexed by a run-time value, so none
// is placed in scratch for that.
#pragma once

#define FX_YERR_JACOBI 5  // `Jacobi iteration unable to converge`

// The first condition raised stays (the word is cleared before the launches): which text comes back does not depend on the order in
// which lanes finish, and a code the assembly has set (1, 2) is not overwritten.
__device__ __forceinline__ void yield_raise(int32_t *err, int code) {
  if (err) atomicCAS(err, 0, code);
}

// position of btens(i, j), i < j, among the three upper off-diagonal terms (0,1) (0,2) (1,2)
__device__ __forceinline__ constexpr int yield_od(int i, int j) { return i + j - 1; }

#define FX_EIGEN3_NAME(x) yield_##x
#define FX_EIGEN3_FP
#include "fx_eigen3_body.h"
#undef FX_EIGEN3_NAME
#undef FX_EIGEN3_FP
#define FX_EIGEN3_NAME(x) exact_##x
#define FX_EIGEN3_FP _Pragma("clang fp contract(off)")
#include "fx_eigen3_body.h"
#undef FX_EIGEN3_NAME
#undef FX_EIGEN3_FP
