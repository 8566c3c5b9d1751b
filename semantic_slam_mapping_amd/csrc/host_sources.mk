# The library's host-only sources, the one list of them: the stages' host-only halves (ssm_host.h), the ORB planner (ssm_orb_plan.h) and the voxel map's protocol
# (ssm_map_plan.h).  Plain C++ without a HIP header: csrc/Makefile compiles them with the library's host compiler and flags into libssm_hip.so, host/Makefile
# compiles them beside san_stub_device.cpp into the programs that do not link the library.  Names are relative to csrc/.
SSM_HOST_SOURCES := ssm_vocab.cpp ssm_vocab_train_host.cpp ssm_uvd_host.cpp ssm_pgo_host.cpp ssm_orb_plan.cpp ssm_map_plan.cpp ssm_motion_fuse_host.cpp ssm_sor_host.cpp ssm_carve_host.cpp ssm_render_host.cpp ssm_align_host.cpp ssm_grid_host.cpp ssm_objects_host.cpp ssm_relabel_host.cpp ssm_cloud_table.cpp ssm_track_host.cpp
