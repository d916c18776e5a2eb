# Build the MI355X library (HIP, gfx950) and the CPU oracle (test infrastructure).
#   make            -> real_time_ray_tracer_amd/librtrt.so and librtrt_mesh.so, oracle/build/librt_oracle.so, build/rt_headless
#   make lib|oracle|headless|clean
#   make b1sort0    -> build/v_b1sort0/librtrt.so: the library with RT_B1_SORT=0 (test infrastructure)
#   make ablib      -> build/librtrt_ab.so: the same shim over tools/ab/rt_kernels_ab.hip, the launcher
#                      with the experimental A/B kernels and their RTRT_* environment switches
#                      (tools/ab.py: RTRT_LIB=build/librtrt_ab.so); never part of librtrt.so
HIPCC    ?= /opt/rocm/bin/hipcc
CC       ?= gcc
ARCH     ?= gfx950
PKG      := real_time_ray_tracer_amd
CSRC     := $(PKG)/csrc
OBJDIR   := build/obj

# -ffp-contract=off + correctly-rounded f32 '/' and sqrt: the float semantics shared with the
# oracle (oracle/rt_oracle.h).  No fast-math anywhere.
HIPFLAGS := -O3 -std=c++17 --offload-arch=$(ARCH) -fPIC -ffp-contract=off $(HIPFLAGS_EXTRA) \
            -fhip-fp32-correctly-rounded-divide-sqrt -fno-slp-vectorize -Wall -Wno-unused-function -Iinclude
CFLAGS_ORACLE := -O3 -march=x86-64-v3 -ffp-contract=off -fopenmp -fPIC -std=c99 -Wall

LIB      := $(PKG)/librtrt.so
# the companion library of include/rt/mesh.h (triangle meshes), next to the production library
MESHLIB   = $(dir $(LIB))librtrt_mesh.so
ORACLE   := oracle/build/librt_oracle.so
ORACLE_NATIVE := oracle/build/librt_oracle_zen.so
HEADLESS := build/rt_headless

all: lib oracle headless
lib: $(LIB) $(MESHLIB)
oracle: $(ORACLE) $(ORACLE_NATIVE)
headless: $(HEADLESS)

# kernels whose leading arguments are scalars (hybrid_kernel's tables, selftest_kernel) get
# them preloaded into SGPRs at wave launch (gfx950 kernarg preload; FrameParams is never preloaded)
KARG_PRELOAD ?= -mllvm -amdgpu-kernarg-preload-count=7

$(OBJDIR)/rt_kernels.o: $(CSRC)/rt_kernels.hip $(CSRC)/*.h include/rt/*.h | $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(KARG_PRELOAD) -x hip -c $< -o $@

$(OBJDIR)/%.o: $(CSRC)/%.hip $(CSRC)/*.h include/rt/*.h | $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -x hip -c $< -o $@

# the host-only units (no HIP header): rt_host.cpp, rt_plan.cpp, rt_query_host.cpp, rt_mesh_host.cpp
$(OBJDIR)/rt_host.o $(OBJDIR)/rt_plan.o $(OBJDIR)/rt_query_host.o $(OBJDIR)/rt_mesh_host.o: $(OBJDIR)/%.o: $(CSRC)/%.cpp $(CSRC)/*.h include/rt/*.h | $(OBJDIR)
	$(HIPCC) -O3 -std=c++17 -fPIC -ffp-contract=off $(HIPFLAGS_EXTRA) -Wall -Iinclude -c $< -o $@

$(OBJDIR)/rt_group.o: $(CSRC)/rt_group.cpp $(CSRC)/rt_kernels.h include/rt/*.h | $(OBJDIR)
	$(HIPCC) -O2 -std=c++17 --offload-arch=$(ARCH) -fPIC -Wall -Iinclude -c $< -o $@

# the shim and its components (rt_stage, rt_sched, rt_cull, rt_gbuf, rt_timing, rt_query, rt_tree), the host-only units, the group
SHIM_OBJS := $(addprefix $(OBJDIR)/,rt_shim.o rt_stage.o rt_sched.o rt_cull.o rt_gbuf.o rt_timing.o rt_query.o rt_tree.o rt_host.o \
               rt_plan.o rt_query_host.o rt_group.o)

# BUILD_INFO: sha1 of the library's sources (+ the git commit they were built at, "+dirty" if
# they differ from it), so measurements can name the kernel code they were taken on
$(LIB): $(OBJDIR)/rt_kernels.o $(SHIM_OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $^ -lpthread
	@src=$$(cat $(CSRC)/*.hip $(CSRC)/*.h $(CSRC)/*.cpp include/rt/*.h Makefile | sha1sum | cut -c1-12); \
	 commit=$$(git rev-parse --short=12 HEAD 2>/dev/null || echo unknown); \
	 git diff --quiet HEAD -- $(CSRC) include Makefile 2>/dev/null || commit="$$commit+dirty"; \
	 printf '{"src_sha1": "%s", "commit": "%s"}\n' "$$src" "$$commit" > $(dir $@)BUILD_INFO

# librtrt_mesh.so: the mesh object, its two kernels and the host-only unit; nothing of librtrt.so's
MESH_OBJS := $(addprefix $(OBJDIR)/,rt_mesh.o rt_mesh_kernels.o rt_mesh_host.o)
$(MESHLIB): $(MESH_OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $^

ABLIB := build/librtrt_ab.so
$(OBJDIR)/rt_kernels_ab.o: tools/ab/rt_kernels_ab.hip $(CSRC)/*.h include/rt/*.h | $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(KARG_PRELOAD) -I$(CSRC) -x hip -c $< -o $@

$(ABLIB): $(OBJDIR)/rt_kernels_ab.o $(SHIM_OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $^ -lpthread

ablib: $(ABLIB)

# The library built with RT_B1_SORT=0 (the AO pools' samples in item order, no sort instantiation
# launched): tests/test_gpu_ao_sort.py compares it with the default build  -> build/v_b1sort0/librtrt.so
b1sort0:
	$(MAKE) variant V=b1sort0 VFLAGS=-DRT_B1_SORT=0

# A compile-time variant of the production library for tools/ab.py --libs (same sources, extra
# defines):  make variant V=post32x8 VFLAGS="-DRT_POST_BWX=4 -DRT_POST_BWY=1"  -> build/v_post32x8/librtrt.so
variant:
	$(MAKE) build/v_$(V)/librtrt.so OBJDIR=build/v_$(V)/obj LIB=build/v_$(V)/librtrt.so HIPFLAGS_EXTRA="$(VFLAGS)"

$(ORACLE): oracle/rt_oracle.c oracle/rt_oracle.h include/rt/layout.h
	@mkdir -p oracle/build
	$(CC) $(CFLAGS_ORACLE) -shared -o $@ oracle/rt_oracle.c -lquadmath -lm

# CPU-baseline build for the GPU box's AMD EPYC (Zen 5) host cores; same source and float flags
$(ORACLE_NATIVE): oracle/rt_oracle.c oracle/rt_oracle.h include/rt/layout.h
	@mkdir -p oracle/build
	$(CC) $(subst -march=x86-64-v3,-march=znver3 -mtune=znver3 -mavx512f -mavx512cd -mavx512bw -mavx512dq -mavx512vl,$(CFLAGS_ORACLE)) -shared -o $@ oracle/rt_oracle.c -lquadmath -lm

$(HEADLESS): $(CSRC)/rt_headless.cpp $(LIB) $(MESHLIB) include/rt/*.h
	$(CXX) -O2 -std=c++17 -Iinclude -o $@ $< -L$(PKG) -lrtrt -lrtrt_mesh -Wl,-rpath,'$$ORIGIN/../$(PKG)'

$(OBJDIR):
	@mkdir -p $(OBJDIR)

clean:
	rm -rf build oracle/build $(LIB) $(MESHLIB)

.PHONY: all lib oracle headless ablib variant b1sort0 clean
