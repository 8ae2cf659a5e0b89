// irm_launch_decl.hpp — declarations of the per-shape launcher templates and the lists of shapes that have
// an instantiation unit (IRM_FIX_SHAPES, IRM_EXTERN_*; build.py FIX_SHAPES).  Host code only.
// Included by irm_kernels.hip, which dispatches into the instantiation units without compiling a kernel of
// theirs, and by irm_kernels_impl.hpp, which defines the templates.
#pragma once
#include <hip/hip_runtime.h>

#include "irm_kernels.hpp"
#include "irm_opt_common.hpp"  // the shapes the IRM_EXTERN_* lists name

namespace irm {

// The per-shape launchers (defined in irm_kernels_impl.hpp): the lean / general dispatch of one shape, the dense
// operator's k_lean (*served = false leaves the launch to the general kernel) and k_forward of one D.
template <class Sh>
hipError_t launch_optimize_shape(const KParams& p, hipStream_t s, LaunchDesc* desc);
template <class Sh>
hipError_t launch_dense_shape(const KParams& p, hipStream_t s, LaunchDesc* desc, bool* served);
template <int D>
hipError_t launch_forward_dim(const KParams& p, int mode, hipStream_t s);

// Instantiated in irm_opt_inst.hip (IRM_INST_* macros); irm_kernels.hip only dispatches.
#define IRM_FIX_SHAPES(X) X(3, 50) X(3, 64) X(3, 128) X(3, 256) X(7, 128) X(7, 256)
#define IRM_EXTERN_FIX(D_, N_) \
    extern template hipError_t launch_optimize_shape<FixShape<D_, N_, 32>>(const KParams&, hipStream_t, LaunchDesc*);
#define IRM_EXTERN_DENSE(D_, N_) \
    extern template hipError_t launch_dense_shape<DenseShape<D_, N_>>(const KParams&, hipStream_t, LaunchDesc*, bool*);
#define IRM_EXTERN_DYN(D_)                                                                                      \
    extern template hipError_t launch_optimize_shape<DynShape<D_>>(const KParams&, hipStream_t, LaunchDesc*); \
    extern template hipError_t launch_forward_dim<D_>(const KParams&, int, hipStream_t);

}  // namespace irm
