# Builds the C-ABI library without Python (the same command dvo_slam_amd/_build.py runs) and the oracle (test infrastructure).
HIPCC ?= /opt/rocm/bin/hipcc
SRC   := dvo_slam_amd/csrc
LIB   := dvo_slam_amd/libdvo_amd.so
FLAGS := $(shell python3 dvo_slam_amd/_build.py --print-flags)
BUILD_ID := $(shell python3 dvo_slam_amd/_build.py --print-id)

all: $(LIB)

CPP := $(SRC)/dvo_kernels.hip $(SRC)/dvo_pyramid.cpp $(SRC)/dvo_tracker.cpp $(SRC)/dvo_sharded.cpp $(SRC)/dvo_probes.cpp \
       $(SRC)/dvo_validator.cpp $(SRC)/dvo_frontend.cpp $(SRC)/dvo_tum.cpp $(SRC)/dvo_map.cpp $(SRC)/dvo_graph.cpp \
       $(SRC)/dvo_graph_batch.cpp $(SRC)/dvo_covisibility.cpp $(SRC)/dvo_rectify.cpp $(SRC)/dvo_register.cpp \
       $(SRC)/dvo_ingest.cpp $(SRC)/dvo_mask.cpp $(SRC)/dvo_budget.cpp $(SRC)/dvo_mask_ops.cpp \
       $(SRC)/dvo_mask_residual.cpp $(SRC)/dvo_fuse.cpp $(SRC)/dvo_place.cpp $(SRC)/dvo_normals.cpp \
       $(SRC)/dvo_depth_filter.cpp $(SRC)/dvo_components.cpp $(SRC)/dvo_pose_score.cpp \
       $(SRC)/dvo_exposure.cpp $(SRC)/dvo_warp.cpp $(SRC)/dvo_volume.cpp

$(LIB): $(CPP) $(SRC)/dvo_types.h $(SRC)/dvo_internal.h $(SRC)/se3.h $(SRC)/dvo_graph_device.h $(SRC)/dvo_graph_host.h \
        $(SRC)/dvo_components_core.h $(SRC)/dvo_exposure_solve.h $(SRC)/dvo_volume_box.h $(SRC)/dvo_launch_rules.h \
        $(SRC)/dvo_call.h $(SRC)/dvo_device_rules.h include/dvo_amd.h include/dvo_amd_debug.h
	$(HIPCC) $(FLAGS) '-DDVO_AMD_BUILD_ID="$(BUILD_ID)"' -x hip $(CPP) -lz -o $@

oracle:
	$(MAKE) -C oracle

# the C examples that need no input files, and budget_selection_example, mask_ops_example, residual_mask_example, depth_fusion_example, place_index_example, the two normals examples, the two depth_filter examples the two mask_components examples, the two pose_scoring examples and the two exposure examples, which take their frames as float32 files (the tests
# build every example themselves, tests/test_*_adaptor.py)
examples: $(LIB)
	mkdir -p examples/_build
	$(CC) -std=c99 -Wall -Iinclude examples/keyframe_map_example.c -o examples/_build/keyframe_map_example \
	    -Ldvo_slam_amd -ldvo_amd -Wl,-rpath,$(CURDIR)/dvo_slam_amd -Wl,--allow-shlib-undefined
	$(CC) -std=c99 -Wall -Iinclude examples/constraint_search_example.c -o examples/_build/constraint_search_example \
	    -Ldvo_slam_amd -ldvo_amd -lm -Wl,-rpath,$(CURDIR)/dvo_slam_amd -Wl,--allow-shlib-undefined
	$(CC) -std=c99 -Wall -Iinclude examples/rectified_ingest_example.c -o examples/_build/rectified_ingest_example \
	    -Ldvo_slam_amd -ldvo_amd -Wl,-rpath,$(CURDIR)/dvo_slam_amd -Wl,--allow-shlib-undefined
	$(CC) -std=c99 -Wall -Iinclude examples/registered_ingest_example.c -o examples/_build/registered_ingest_example \
	    -Ldvo_slam_amd -ldvo_amd -Wl,-rpath,$(CURDIR)/dvo_slam_amd -Wl,--allow-shlib-undefined
	$(CC) -std=c99 -Wall -Iinclude examples/batch_ingest_example.c -o examples/_build/batch_ingest_example \
	    -Ldvo_slam_amd -ldvo_amd -Wl,-rpath,$(CURDIR)/dvo_slam_amd -Wl,--allow-shlib-undefined
	$(CC) -std=c99 -Wall -Iinclude examples/budget_selection_example.c -o examples/_build/budget_selection_example \
	    -Ldvo_slam_amd -ldvo_amd -Wl,-rpath,$(CURDIR)/dvo_slam_amd -Wl,--allow-shlib-undefined
	$(CC) -std=c99 -Wall -Iinclude examples/mask_ops_example.c -o examples/_build/mask_ops_example \
	    -Ldvo_slam_amd -ldvo_amd -Wl,-rpath,$(CURDIR)/dvo_slam_amd -Wl,--allow-shlib-undefined
	$(CC) -std=c99 -Wall -Iinclude examples/residual_mask_example.c -o examples/_build/residual_mask_example \
	    -Ldvo_slam_amd -ldvo_amd -Wl,-rpath,$(CURDIR)/dvo_slam_amd -Wl,--allow-shlib-undefined
	$(CC) -std=c99 -Wall -Iinclude examples/depth_fusion_example.c -o examples/_build/depth_fusion_example \
	    -Ldvo_slam_amd -ldvo_amd -Wl,-rpath,$(CURDIR)/dvo_slam_amd -Wl,--allow-shlib-undefined
	$(CC) -std=c99 -Wall -Iinclude examples/place_index_example.c -o examples/_build/place_index_example \
	    -Ldvo_slam_amd -ldvo_amd -Wl,-rpath,$(CURDIR)/dvo_slam_amd -Wl,--allow-shlib-undefined
	$(CC) -std=c99 -Wall -Iinclude examples/normals_example.c -o examples/_build/normals_example \
	    -Ldvo_slam_amd -ldvo_amd -Wl,-rpath,$(CURDIR)/dvo_slam_amd -Wl,--allow-shlib-undefined
	$(CXX) -std=c++11 -Wall -pthread -Iinclude/dvo_amd_compat -Iinclude examples/normals_adaptor_example.cpp \
	    -o examples/_build/normals_adaptor_example -Ldvo_slam_amd -ldvo_amd -Wl,-rpath,$(CURDIR)/dvo_slam_amd -Wl,--allow-shlib-undefined
	$(CC) -std=c99 -Wall -Iinclude examples/depth_filter_example.c -o examples/_build/depth_filter_example \
	    -Ldvo_slam_amd -ldvo_amd -Wl,-rpath,$(CURDIR)/dvo_slam_amd -Wl,--allow-shlib-undefined
	$(CXX) -std=c++11 -Wall -pthread -Iinclude/dvo_amd_compat -Iinclude examples/depth_filter_adaptor_example.cpp \
	    -o examples/_build/depth_filter_adaptor_example -Ldvo_slam_amd -ldvo_amd -Wl,-rpath,$(CURDIR)/dvo_slam_amd -Wl,--allow-shlib-undefined
	$(CC) -std=c99 -Wall -Iinclude examples/mask_components_example.c -o examples/_build/mask_components_example \
	    -Ldvo_slam_amd -ldvo_amd -Wl,-rpath,$(CURDIR)/dvo_slam_amd -Wl,--allow-shlib-undefined
	$(CXX) -std=c++11 -Wall -pthread -Iinclude/dvo_amd_compat -Iinclude examples/mask_components_adaptor_example.cpp \
	    -o examples/_build/mask_components_adaptor_example -Ldvo_slam_amd -ldvo_amd -Wl,-rpath,$(CURDIR)/dvo_slam_amd -Wl,--allow-shlib-undefined
	$(CC) -std=c99 -Wall -Iinclude examples/pose_scoring_example.c -o examples/_build/pose_scoring_example \
	    -Ldvo_slam_amd -ldvo_amd -Wl,-rpath,$(CURDIR)/dvo_slam_amd -Wl,--allow-shlib-undefined
	$(CXX) -std=c++11 -Wall -pthread -Iinclude/dvo_amd_compat -Iinclude examples/pose_scoring_adaptor_example.cpp \
	    -o examples/_build/pose_scoring_adaptor_example -Ldvo_slam_amd -ldvo_amd -Wl,-rpath,$(CURDIR)/dvo_slam_amd -Wl,--allow-shlib-undefined
	$(CC) -std=c99 -Wall -Iinclude examples/exposure_example.c -o examples/_build/exposure_example \
	    -Ldvo_slam_amd -ldvo_amd -Wl,-rpath,$(CURDIR)/dvo_slam_amd -Wl,--allow-shlib-undefined
	$(CXX) -std=c++11 -Wall -pthread -Iinclude/dvo_amd_compat -Iinclude examples/exposure_adaptor_example.cpp \
	    -o examples/_build/exposure_adaptor_example -Ldvo_slam_amd -ldvo_amd -Wl,-rpath,$(CURDIR)/dvo_slam_amd -Wl,--allow-shlib-undefined
	$(CC) -std=c99 -Wall -Iinclude examples/frame_warp_example.c -o examples/_build/frame_warp_example \
	    -Ldvo_slam_amd -ldvo_amd -Wl,-rpath,$(CURDIR)/dvo_slam_amd -Wl,--allow-shlib-undefined
	$(CXX) -std=c++11 -Wall -pthread -Iinclude/dvo_amd_compat -Iinclude examples/frame_warp_adaptor_example.cpp \
	    -o examples/_build/frame_warp_adaptor_example -Ldvo_slam_amd -ldvo_amd -Wl,-rpath,$(CURDIR)/dvo_slam_amd -Wl,--allow-shlib-undefined
	$(CC) -std=c99 -Wall -Iinclude examples/volume_example.c -o examples/_build/volume_example \
	    -Ldvo_slam_amd -ldvo_amd -Wl,-rpath,$(CURDIR)/dvo_slam_amd -Wl,--allow-shlib-undefined
	$(CXX) -std=c++11 -Wall -pthread -Iinclude/dvo_amd_compat -Iinclude examples/volume_adaptor_example.cpp \
	    -o examples/_build/volume_adaptor_example -Ldvo_slam_amd -ldvo_amd -Wl,-rpath,$(CURDIR)/dvo_slam_amd -Wl,--allow-shlib-undefined
	$(CC) -std=c99 -Wall -Iinclude examples/volume_mesh_example.c -o examples/_build/volume_mesh_example \
	    -Ldvo_slam_amd -ldvo_amd -Wl,-rpath,$(CURDIR)/dvo_slam_amd -Wl,--allow-shlib-undefined
	$(CXX) -std=c++11 -Wall -pthread -Iinclude/dvo_amd_compat -Iinclude examples/volume_mesh_adaptor_example.cpp \
	    -o examples/_build/volume_mesh_adaptor_example -Ldvo_slam_amd -ldvo_amd -Wl,-rpath,$(CURDIR)/dvo_slam_amd -Wl,--allow-shlib-undefined

clean:
	rm -f $(LIB)

.PHONY: all oracle examples clean
