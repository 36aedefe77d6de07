# Builds the gfx950 HIP library of the YOLOv11 inference path in-tree.
#   make            -> yolo-infer-pt_amd/yolo_hip/libyolo_hip.so
#   make oracle     -> oracle/_c/liboracle_nms.so (CPU checker, tests only)
ROCM ?= /opt/rocm
HIPCC ?= $(ROCM)/bin/hipcc
ARCH ?= gfx950
PKG := yolo-infer-pt_amd
SRC := $(PKG)/csrc
OUT ?= $(PKG)/yolo_hip/libyolo_hip.so
OBJDIR ?= build/obj
HIPFLAGS := --offload-arch=$(ARCH) -O3 -fPIC -std=c++17 -Iinclude -I$(SRC) \
            -fhip-fp32-correctly-rounded-divide-sqrt -Wno-unused-result $(EXTRA)

# the host runtime behind the handle (net.h) and its C ABI, compiled as HIP
NET := engine net_build net_weights net_forward net_launch net_debug
# handle-free host code compiled as HIP
HOSTHIP := post_abi nms_host
# kernels; the NOFMA ones promise bit-exact arithmetic against host code: no FMA contraction
KERNELS := conv sppf attn decode conv_mx conv_rw head c3k2 c3k pwchain cls
KERNELS_NOFMA := preprocess nms match merge track reid gallery assign motion
# HIP-free translation units: plain C++, no device pass, no FMA contraction
HOSTCXX := match_host merge_host track_host gallery_host assign_host motion_host

objs = $(patsubst %,$(OBJDIR)/%.o,$(1))
OBJS := $(call objs,$(NET) $(HOSTHIP) $(KERNELS) $(KERNELS_NOFMA) $(HOSTCXX))
HOST_H := $(SRC)/host_util.h $(SRC)/host_parallel.h $(SRC)/box_math.h \
          $(SRC)/match_host.h $(SRC)/merge_host.h $(SRC)/track_host.h $(SRC)/gallery_host.h \
          $(SRC)/assign_host.h $(SRC)/motion_host.h

all: $(OUT)

$(OBJDIR):
	mkdir -p $(OBJDIR)

$(call objs,$(NET)): $(OBJDIR)/%.o: $(SRC)/%.cpp $(SRC)/net.h $(SRC)/host_util.h $(SRC)/common.h $(SRC)/conv_mx.h include/yolo_hip.h | $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -x hip -c $< -o $@

$(call objs,$(HOSTHIP)): $(OBJDIR)/%.o: $(SRC)/%.cpp $(SRC)/common.h $(HOST_H) include/yolo_hip.h | $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -x hip -c $< -o $@

$(call objs,$(KERNELS)): $(OBJDIR)/%.o: $(SRC)/%.hip $(SRC)/common.h $(SRC)/dtypes.h $(SRC)/mfma32.h $(SRC)/conv_mx.h include/yolo_hip.h | $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(call objs,$(KERNELS_NOFMA)): $(OBJDIR)/%.o: $(SRC)/%.hip $(SRC)/common.h $(SRC)/dtypes.h include/yolo_hip.h | $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -ffp-contract=off -c $< -o $@

$(call objs,$(HOSTCXX)): $(OBJDIR)/%.o: $(SRC)/%.cpp $(SRC)/%.h $(SRC)/box_math.h $(SRC)/host_parallel.h include/yolo_hip.h | $(OBJDIR)
	$(HIPCC) -x c++ -O3 -fPIC -std=c++17 -Iinclude -I$(SRC) -ffp-contract=off -c $< -o $@

# headers only some units of a group include
# the decode's value arithmetic, shared by its kernels and the fused head's
$(call objs,decode head): $(SRC)/head_math.h
# each shares its arithmetic with its host twin through box_math.h and the twin's header
$(call objs,match merge track motion): $(OBJDIR)/%.o: $(SRC)/%_host.h $(SRC)/box_math.h
# the appearance kernels share the tracker's header: the twins live in track_host.cpp
$(OBJDIR)/reid.o: $(SRC)/track_host.h $(SRC)/box_math.h
# the int8 MFMA kernels share their fragment loads and lane map; the search shares its candidate
# order, chunking and workspace layout with its host twin, which borrows the reid dim check
$(call objs,reid gallery): $(SRC)/mfma_i8.h
$(OBJDIR)/gallery.o: $(SRC)/gallery_host.h $(SRC)/box_math.h
$(OBJDIR)/gallery_host.o: $(SRC)/track_host.h
# the assignment solver: the kernel and the tracker's optimal instances share assign.h, the host
# twins of both share assign_host.h (which also holds the weight arithmetic of all four)
$(call objs,assign track): $(SRC)/assign.h $(SRC)/assign_host.h
$(OBJDIR)/assign.o: $(SRC)/box_math.h
$(OBJDIR)/track_host.o: $(SRC)/assign_host.h
# reports its argument errors through host_util.h's guarded(); its host functions use the pool
$(OBJDIR)/preprocess.o: $(SRC)/host_util.h $(SRC)/host_parallel.h

$(OUT): $(OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(OBJS)

clean:
	rm -rf build $(OUT)

.PHONY: all clean
