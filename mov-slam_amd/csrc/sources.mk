# The sources of libmovba, listed once.  Included by csrc/Makefile (the library and its test build; scripts/build_variant.sh
# goes through it), by tests/hipstub/Makefile and tests/two_view_lo/Makefile (the host side alone, against the stand-in runtime and
# the fake device) and by tests/init_map/Makefile (the same plus MOVBA_HOST_SRCS_OWN_FAKE and that directory's fake launch) and
# by tests/view_points/Makefile (MOVBA_HOST_SRCS plus MOVBA_HOST_SRCS_VIEW and its own fake launch) and by
# tests/point_normals/Makefile (MOVBA_HOST_SRCS plus MOVBA_HOST_SRCS_NORMALS and its own fake launch) and by
# tests/covisibility/Makefile (MOVBA_HOST_SRCS plus MOVBA_HOST_SRCS_COVIS and its own fake launch) and by
# tests/track_match/Makefile (MOVBA_HOST_SRCS plus MOVBA_HOST_SRCS_TRACK and its own fake launch) and by
# tests/express/Makefile (MOVBA_HOST_SRCS plus MOVBA_HOST_SRCS_EXPRESS and its own fake launch) and by
# tests/advance/Makefile (MOVBA_HOST_SRCS plus MOVBA_HOST_SRCS_ADVANCE and its own fake launch) and by
# tests/mv_raster/Makefile (MOVBA_HOST_SRCS plus MOVBA_HOST_SRCS_MVRASTER and its own fake launch) and by
# tests/lk/Makefile (MOVBA_HOST_SRCS plus MOVBA_HOST_SRCS_LK and its own fake launch) and by
# tests/stereo_points/Makefile (MOVBA_HOST_SRCS plus MOVBA_HOST_SRCS_STEREO and its own fake launch).
MOVBA_HIP_SRCS  := kernels.hip pcg_kernel.hip band_kernel.hip dense_solve.hip dense_persist.hip struct_kernels.hip struct_sort.hip \
                   pose_kernels.hip marginals.hip triangulate.hip two_view.hip init_map.hip view_points.hip point_normals.hip \
                   covisibility.hip track_match.hip express.hip advance.hip mv_raster.hip lk.hip stereo_points.hip
MOVBA_HOST_SRCS := api.cpp upload.cpp structure.cpp dense_plan.cpp pcg_plan.cpp pose_opt.cpp marginals.cpp triangulate.cpp two_view.cpp
# host sources whose launch the shared fake device does not stand in for: part of both libraries (csrc/Makefile), not of the
# host-side builds that link MOVBA_HOST_SRCS against tests/hipstub's fixed set of fake launches (tests/init_map has its own)
MOVBA_HOST_SRCS_OWN_FAKE := init_map.cpp
# the same for movba_view_points: a list of its own, because tests/init_map links MOVBA_HOST_SRCS_OWN_FAKE against that directory's
# one fake launch (tests/view_points has the fake launch of this one)
MOVBA_HOST_SRCS_VIEW := view_points.cpp
# and for movba_point_normals / movba_lba_point_normals (tests/point_normals has their fake launch)
MOVBA_HOST_SRCS_NORMALS := point_normals.cpp
# and for movba_covisibility (tests/covisibility has its fake launch)
MOVBA_HOST_SRCS_COVIS := covisibility.cpp
# and for movba_track_match (tests/track_match has its fake launch)
MOVBA_HOST_SRCS_TRACK := track_match.cpp
# and for movba_express (tests/express has its fake launch)
MOVBA_HOST_SRCS_EXPRESS := express.cpp
# and for movba_advance (tests/advance has its fake launch)
MOVBA_HOST_SRCS_ADVANCE := advance.cpp
# and for movba_mv_raster (tests/mv_raster has its fake launch)
MOVBA_HOST_SRCS_MVRASTER := mv_raster.cpp
# and for movba_lk_track (tests/lk has its fake launch)
MOVBA_HOST_SRCS_LK := lk.cpp
# and for movba_stereo_points (tests/stereo_points has its fake launch)
MOVBA_HOST_SRCS_STEREO := stereo_points.cpp
# host sources with a kernel file of the same stem: the kernels' object is <stem>_kernels.o
MOVBA_SAME_STEM := marginals triangulate two_view init_map view_points point_normals covisibility track_match express advance mv_raster lk stereo_points
