# Build libpmx_hip.so (HIP kernels + C ABI) for gfx950, and the CPU oracle (test infrastructure).
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
CSRC := pharmsol_amd/csrc
LIB := pharmsol_amd/lib/libpmx_hip.so
# -ffp-contract=off on the HOST side: the population compiler must evaluate covariate
# lines (slope*t + intercept) exactly like the reference; device code keeps FMA contraction.
HOSTFLAGS := -O2 -std=c++17 -fPIC -Wall -Wextra -ffp-contract=off -Iinclude
DEVFLAGS := -O3 -std=c++17 -fPIC --offload-arch=$(ARCH) -Wall -Wno-unused-parameter -Iinclude
# the kernel units: one translation unit per kernel family (pmx_lanes.hpp lists them)
KUNITS := pmx_grid pmx_dyn3 pmx_steps pmx_pair pmx_classed pmx_classed_ll pmx_ode_builtin pmx_util pmx_mixture pmx_posterior pmx_exposure
OBJ := $(CSRC)/build/pmx_compile.o $(CSRC)/build/pmx_plan.o $(CSRC)/build/pmx_api.o $(CSRC)/build/pmx_model.o $(CSRC)/build/pmx_host.o $(CSRC)/build/pmx_stream.o $(CSRC)/build/pmx_launch.o $(KUNITS:%=$(CSRC)/build/%.o) $(CSRC)/build/pmx_jit.o $(CSRC)/build/pmx_jit_source.o $(CSRC)/build/pmx_jit_cache.o $(CSRC)/build/pmx_alloc.o $(CSRC)/build/pmx_shard.o
DEVHDR := $(CSRC)/pmx_devtypes.hpp $(CSRC)/pmx_device.hpp $(CSRC)/pmx_ode.hpp $(CSRC)/pmx_structures.hpp $(CSRC)/pmx_userlag.hpp $(CSRC)/pmx_analytical.hpp $(CSRC)/pmx_ode_user.hpp include/pmx.h

all: $(LIB) oracle

# the population compiler: pure host code (pmx_compile.cpp: population and op stream; pmx_plan.cpp: class plan, records)
PLANSRC := $(CSRC)/pmx_compile.cpp $(CSRC)/pmx_plan.cpp
PLANHDR := $(CSRC)/pmx_compile.hpp $(CSRC)/pmx_devtypes.hpp include/pmx.h
$(CSRC)/build/pmx_compile.o $(CSRC)/build/pmx_plan.o: $(CSRC)/build/%.o: $(CSRC)/%.cpp $(PLANHDR)
	@mkdir -p $(CSRC)/build
	g++ $(HOSTFLAGS) -c $< -o $@

# the C ABI's translation units (pmx_internal.hpp): entry points, device streams, launch path, code-object cache
APIHDR := $(CSRC)/pmx_internal.hpp $(CSRC)/pmx_jit_cache.hpp $(CSRC)/pmx_compile.hpp $(CSRC)/pmx_kernels.hpp $(CSRC)/pmx_structures.hpp $(CSRC)/pmx_jit.hpp $(CSRC)/pmx_jit_source.hpp $(CSRC)/pmx_solvers.hpp $(DEVHDR)
$(CSRC)/build/pmx_api.o $(CSRC)/build/pmx_model.o $(CSRC)/build/pmx_host.o $(CSRC)/build/pmx_stream.o $(CSRC)/build/pmx_launch.o $(CSRC)/build/pmx_jit_cache.o: $(CSRC)/build/%.o: $(CSRC)/%.cpp $(APIHDR)
	@mkdir -p $(CSRC)/build
	$(HIPCC) $(DEVFLAGS) -ffp-contract=off -x hip -c $< -o $@

KHDR := $(CSRC)/pmx_lanes.hpp $(CSRC)/pmx_kernels.hpp $(CSRC)/pmx_weights.hpp $(CSRC)/pmx_solvers.hpp $(CSRC)/pmx_compile.hpp $(DEVHDR)
$(CSRC)/build/%.o: $(CSRC)/%.hip $(KHDR)
	@mkdir -p $(CSRC)/build
	$(HIPCC) $(DEVFLAGS) -c $< -o $@

# a kernel unit's device assembly, same flags (tools/isa_guard.py, isa_count.sh, isa_of.py, kernel_resources.py); `make asm`: all units
$(CSRC)/build/%.s: $(CSRC)/%.hip $(KHDR)
	@mkdir -p $(CSRC)/build
	$(HIPCC) $(DEVFLAGS) --cuda-device-only -S $< -o $@

asm: $(KUNITS:%=$(CSRC)/build/%.s)

# the device headers a run-time (hiprtc) compile of a user model includes, embedded as string literals
$(CSRC)/build/pmx_jit_headers.inc: $(DEVHDR) tools/embed_headers.py
	@mkdir -p $(CSRC)/build
	python3 tools/embed_headers.py $@ include/pmx.h $(CSRC)/pmx_devtypes.hpp $(CSRC)/pmx_device.hpp $(CSRC)/pmx_ode.hpp $(CSRC)/pmx_structures.hpp $(CSRC)/pmx_userlag.hpp $(CSRC)/pmx_analytical.hpp $(CSRC)/pmx_ode_user.hpp

$(CSRC)/build/pmx_alloc.o: $(CSRC)/pmx_alloc.cpp include/pmx.h
	@mkdir -p $(CSRC)/build
	$(HIPCC) $(DEVFLAGS) -x hip -c $< -o $@

$(CSRC)/build/pmx_shard.o: $(CSRC)/pmx_shard.cpp include/pmx.h
	@mkdir -p $(CSRC)/build
	$(HIPCC) $(DEVFLAGS) -x hip -c $< -o $@

# the text handed to hiprtc (translation units, descriptor-generated closures): pure host code
JITSRC := $(CSRC)/pmx_jit_source.cpp
JITSRCHDR := $(CSRC)/pmx_jit_source.hpp $(CSRC)/pmx_solvers.hpp $(CSRC)/pmx_devtypes.hpp include/pmx.h
$(CSRC)/build/pmx_jit_source.o: $(JITSRC) $(JITSRCHDR)
	@mkdir -p $(CSRC)/build
	g++ $(HOSTFLAGS) -c $< -o $@

$(CSRC)/build/pmx_jit.o: $(CSRC)/pmx_jit.cpp $(CSRC)/pmx_jit.hpp $(JITSRCHDR) $(CSRC)/pmx_jit_cache.hpp $(CSRC)/build/pmx_jit_headers.inc
	$(HIPCC) $(DEVFLAGS) -I$(CSRC)/build -x hip -c $< -o $@

$(LIB): $(OBJ)
	@mkdir -p pharmsol_amd/lib
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(OBJ) -L/opt/rocm/lib -lhiprtc -ldl

oracle:
	$(MAKE) -C oracle

clean:
	rm -rf $(CSRC)/build pharmsol_amd/lib oracle/_build

# the two generated bindings of include/pmx.h (tools/pmx_header.py reads the header for both); run after changing the header
bindings:
	python3 tools/gen_rust_binding.py
	python3 tools/gen_python_binding.py

.PHONY: all oracle clean asm bindings plan_fingerprint plan_fingerprint_san jit_source_fingerprint jit_source_fingerprint_san

# Fingerprint of every array the population compiler produces (tests/test_plan_fingerprint.py compares its output with
# tests/golden/plan_fingerprints.txt).  Host sources only.  FPBIN: where the program goes.  plan_fingerprint_san: the same
# program under AddressSanitizer + UBSan, run stand-alone: `make plan_fingerprint_san && tests/cpp/plan_fingerprint_san`
FPBIN ?= tests/cpp/plan_fingerprint
plan_fingerprint: $(FPBIN)
$(FPBIN): tests/cpp/plan_fingerprint.cpp $(PLANSRC) $(PLANHDR)
	g++ $(HOSTFLAGS) -I$(CSRC) -o $@ tests/cpp/plan_fingerprint.cpp $(PLANSRC)
plan_fingerprint_san: tests/cpp/plan_fingerprint_san
tests/cpp/plan_fingerprint_san: tests/cpp/plan_fingerprint.cpp $(PLANSRC) $(PLANHDR)
	g++ $(HOSTFLAGS) -I$(CSRC) -fsanitize=address,undefined -fno-omit-frame-pointer -o $@ tests/cpp/plan_fingerprint.cpp $(PLANSRC)

# Fingerprint of every text the run-time compilation path generates (tests/test_jit_source_fingerprint.py compares its
# output with tests/golden/jit_source_fingerprints.txt).  Host sources only.  JSFPBIN: where the program goes.
# jit_source_fingerprint_san: `make jit_source_fingerprint_san && tests/cpp/jit_source_fingerprint_san`
JSFPBIN ?= tests/cpp/jit_source_fingerprint
jit_source_fingerprint: $(JSFPBIN)
$(JSFPBIN): tests/cpp/jit_source_fingerprint.cpp $(JITSRC) $(JITSRCHDR)
	g++ $(HOSTFLAGS) -I$(CSRC) -o $@ tests/cpp/jit_source_fingerprint.cpp $(JITSRC)
jit_source_fingerprint_san: tests/cpp/jit_source_fingerprint_san
tests/cpp/jit_source_fingerprint_san: tests/cpp/jit_source_fingerprint.cpp $(JITSRC) $(JITSRCHDR)
	g++ $(HOSTFLAGS) -I$(CSRC) -fsanitize=address,undefined -fno-omit-frame-pointer -o $@ tests/cpp/jit_source_fingerprint.cpp $(JITSRC)

# C++ host-facade test binary (links the product library and, as the checker, the CPU oracle)
tests/cpp/facade_test: tests/cpp/facade_test.cpp include/pharmsol_hip.hpp include/pmx.h $(LIB) oracle
	g++ -O1 -std=c++17 -Wall -Wextra -o $@ tests/cpp/facade_test.cpp -Lpharmsol_amd/lib -lpmx_hip -Loracle/_build -lpmx_oracle \
	    -Wl,-rpath,'$$ORIGIN/../../pharmsol_amd/lib' -Wl,-rpath,'$$ORIGIN/../../oracle/_build' -Wl,-rpath,/opt/rocm/lib

# the façade's exposure / attainment call (tests/test_cpp_exposure.py compares its output with the Python path)
tests/cpp/exposure_facade_test: tests/cpp/exposure_facade_test.cpp include/pharmsol_hip.hpp include/pmx.h $(LIB)
	g++ -O1 -std=c++17 -Wall -Wextra -o $@ tests/cpp/exposure_facade_test.cpp -Lpharmsol_amd/lib -lpmx_hip \
	    -Wl,-rpath,'$$ORIGIN/../../pharmsol_amd/lib' -Wl,-rpath,/opt/rocm/lib
