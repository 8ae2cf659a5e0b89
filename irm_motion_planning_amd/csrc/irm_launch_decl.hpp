// irm_launch_decl.hpp — declarations of the per-shape launcher templates and the lists of shapes that have
// an instantiation unit, one list per family (IRM_FIX_SHAPES, IRM_DENSE_SHAPES, IRM_QUEUE_SHAPES, IRM_DYN_DIMS;
// build.py FIX_SHAPES, DENSE_SHAPES, QUEUE_SHAPES, MAX_D — tests/test_work_queue_host.py compares the two).
// Every extern declaration, dispatch test and shape predicate is made from these lists.  Host code only.
// Included by irm_kernels.hip, which dispatches into the instantiation units without compiling a kernel of
// theirs, and by irm_launch.hpp, which defines the templates.
#pragma once
#include <hip/hip_runtime.h>

#include "irm_kernels.hpp"
#include "irm_opt_common.hpp"  // the shapes the IRM_EXTERN_* lists name

namespace irm {

// The per-shape launchers (defined in irm_launch.hpp): the lean / general dispatch of one shape, the dense
// operator's k_lean (*served = false leaves the launch to the general kernel) and k_forward of one D.
template <class Sh>
hipError_t launch_optimize_shape(const KParams& p, hipStream_t s, LaunchDesc* desc);
template <class Sh>
hipError_t launch_dense_shape(const KParams& p, hipStream_t s, LaunchDesc* desc, bool* served);
template <int D>
hipError_t launch_forward_dim(const KParams& p, int mode, hipStream_t s);

// Instantiated in irm_opt_inst.hip (IRM_INST_* macros); irm_kernels.hip only dispatches.
// (D, N) of the shape-specialised kernels at the auto rank R = 32: dispatch + k_lean and the general k_optimize
#define IRM_FIX_SHAPES(X) X(3, 50) X(3, 64) X(3, 128) X(3, 256) X(7, 128) X(7, 256)
// (D, N) of the dense operator's k_lean (DenseShape)
#define IRM_DENSE_SHAPES(X) X(7, 256)
// (D, N) of the work queue's k_lean (units of their own; each is a fixed shape too)
#define IRM_QUEUE_SHAPES(X) X(3, 50) X(3, 64) X(3, 128) X(7, 128)
// D of the DynShape kernels and k_forward: 1 … 8 (build.py MAX_D, dispatch_d)
#define IRM_DYN_DIMS(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8)
#define IRM_EXTERN_FIX(D_, N_) \
    extern template hipError_t launch_optimize_shape<FixShape<D_, N_, 32>>(const KParams&, hipStream_t, LaunchDesc*);
#define IRM_EXTERN_DENSE(D_, N_) \
    extern template hipError_t launch_dense_shape<DenseShape<D_, N_>>(const KParams&, hipStream_t, LaunchDesc*, bool*);
#define IRM_EXTERN_DYN(D_)                                                                                      \
    extern template hipError_t launch_optimize_shape<DynShape<D_>>(const KParams&, hipStream_t, LaunchDesc*); \
    extern template hipError_t launch_forward_dim<D_>(const KParams&, int, hipStream_t);

}  // namespace irm
