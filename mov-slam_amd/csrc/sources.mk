# The sources of libmovba, listed once.  Included by csrc/Makefile (the library and its test build; scripts/build_variant.sh
# goes through it) and by tests/hipstub/Makefile (the host side alone, against the stand-in runtime and the fake device).
MOVBA_HIP_SRCS  := kernels.hip pcg_kernel.hip band_kernel.hip dense_solve.hip dense_persist.hip struct_kernels.hip struct_sort.hip \
                   pose_kernels.hip marginals.hip triangulate.hip two_view.hip
MOVBA_HOST_SRCS := api.cpp upload.cpp structure.cpp dense_plan.cpp pcg_plan.cpp pose_opt.cpp marginals.cpp triangulate.cpp two_view.cpp
# host sources with a kernel file of the same stem: the kernels' object is <stem>_kernels.o
MOVBA_SAME_STEM := marginals triangulate two_view
