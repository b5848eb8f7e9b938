# Build the ft_sgemm CLI binary and the torch extension (gfx950 only).
HIPCC ?= hipcc
ARCH  ?= gfx950
ROCM  ?= /opt/rocm

all: gen cli ext

gen:
	python3 csrc/codegen/gen_kernels.py

cli: bin/ft_sgemm

# filter out PyTorch-hipify byproducts (kernel_*_hip.hip copies)
KERNEL_TUS := $(filter-out %_hip.hip, $(wildcard csrc/generated/kernel_*.hip))

CLI_SRCS := csrc/cli_main.hip csrc/dispatch.hip csrc/rocblas_path.hip \
            csrc/locate_selftest.hip $(KERNEL_TUS)
CLI_HIPCC = $(HIPCC) -x hip --offload-arch=$(ARCH) -O3 -std=c++17 -Icsrc
CLI_LIBS := -L$(ROCM)/lib -lrocblas -lroctx64

bin/ft_sgemm: $(CLI_SRCS) csrc/ft_kernels.hpp csrc/ft_streamk.hpp csrc/ft_ragged.hpp csrc/ft_ragged_streamk.hpp csrc/ft_ragged_grouped_streamk.hpp csrc/tier_launch.hpp csrc/ft_core.h csrc/fault_log.h csrc/grouped_table.h csrc/generated/tile_params.h
	mkdir -p bin
	$(CLI_HIPCC) $(FTFLAGS) $(CLI_SRCS) $(CLI_LIBS) -o $@

# Paranoid-sync build for the race check (tools/race_check.sh): every
# async-staging site gets an immediate full vmcnt/lgkm drain + barrier;
# outputs must be BIT-IDENTICAL to the normal build (same per-thread
# arithmetic order) — any difference indicates a staging race.
cli-paranoid:
	mkdir -p bin
	$(CLI_HIPCC) -DFT_PARANOID $(CLI_SRCS) $(CLI_LIBS) -o bin/ft_sgemm_paranoid

ext:
	# ninja does not track header deps for hipcc sources: rebuild .hip TUs
	# whenever a csrc header is newer than the built extension
	@SO=$$(ls -t ft_sgemm_amd/_C*.so 2>/dev/null | head -1); \
	if [ -n "$$SO" ] && [ -n "$$(find csrc \( -name '*.hpp' -o -name '*.h' \) -newer $$SO 2>/dev/null)" ]; then touch csrc/*.hip csrc/generated/*.hip; fi
	PYTORCH_ROCM_ARCH=$(ARCH) python3 setup.py build_ext --inplace

clean:
	rm -rf bin build ft_sgemm_amd/_C*.so

.PHONY: all gen cli ext clean
