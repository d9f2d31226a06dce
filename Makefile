# Build of the MI355X topic-routing engine (gfx950 only) and its test oracle.
#   emqx_amd/libtopicmatch.so  product: C-ABI + HIP kernels (hipcc, gfx950)
#   emqx_amd/libtmwork.so      synthetic workload generator (bench/test input)
#   oracle/liboracle.so        CPU restatement of the reference (checker only)
HIPCC   ?= /opt/rocm/bin/hipcc
ARCH    ?= gfx950
CC      ?= gcc
TMDEFS  ?=
HIPFLAGS = --offload-arch=$(ARCH) -O3 -fPIC -std=c++17 -Wall -Wno-unused-result $(TMDEFS)
BUILD   ?= build
LIBOUT  ?= emqx_amd/libtopicmatch.so

all: $(LIBOUT) emqx_amd/libtmwork.so oracle/liboracle.so tools/ubench/batcher_bench tools/ubench/libbatchdrive.so tools/ubench/libpubdrive.so tools/ubench/libinboxdrive.so tools/ubench/libfwddrive.so

$(BUILD):
	mkdir -p $(BUILD)

# every kernel file: one rule (device_bytes.h is the shared device header)
$(BUILD)/%.o: emqx_amd/csrc/%.hip emqx_amd/csrc/kernels.h emqx_amd/csrc/image.h emqx_amd/csrc/device_bytes.h emqx_amd/csrc/deliver.h include/topicmatch.h | $(BUILD)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(BUILD)/engine.o: emqx_amd/csrc/engine.cpp emqx_amd/csrc/kernels.h emqx_amd/csrc/image.h emqx_amd/csrc/deliver.h include/topicmatch.h | $(BUILD)
	$(HIPCC) -O3 -fPIC -std=c++17 -Wall $(TMDEFS) -c $< -o $@

# A/B builds of compile-time variants: make variant TAG=x TMDEFS="-D..." ->
# emqx_amd/variants/libtopicmatch_x.so (bench.py --lib)
variant:
	mkdir -p emqx_amd/variants
	$(MAKE) BUILD=build_$(TAG) LIBOUT=emqx_amd/variants/libtopicmatch_$(TAG).so TMDEFS="$(TMDEFS)" emqx_amd/variants/libtopicmatch_$(TAG).so
.PHONY: variant

$(BUILD)/exchange.o: emqx_amd/csrc/exchange.cpp emqx_amd/csrc/kernels.h include/topicmatch.h | $(BUILD)
	$(HIPCC) -O2 -fPIC -std=c++17 -Wall -c $< -o $@

$(BUILD)/batcher.o: emqx_amd/csrc/batcher.cpp emqx_amd/csrc/batcher_layout.h include/topicmatch.h | $(BUILD)
	$(HIPCC) -O2 -fPIC -std=c++17 -Wall -pthread -c $< -o $@

LIBOBJS = $(BUILD)/kernels.o $(BUILD)/shard.o $(BUILD)/route.o $(BUILD)/routes.o $(BUILD)/presort.o $(BUILD)/aggre.o $(BUILD)/dispatch.o $(BUILD)/share.o $(BUILD)/forward.o $(BUILD)/inbox.o $(BUILD)/pack.o $(BUILD)/engine.o $(BUILD)/batcher.o $(BUILD)/acl.o $(BUILD)/admit.o $(BUILD)/rewrite.o $(BUILD)/exchange.o
$(LIBOUT): $(LIBOBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -pthread $^ -L/opt/rocm/lib -lrccl -o $@

emqx_amd/libtmwork.so: emqx_amd/csrc/workload.c
	$(CC) -O2 -fPIC -shared -Wall $< -o $@ -lm

oracle/liboracle.so: oracle/o1_trie.c oracle/o3_interned.c
	$(CC) -O2 -fPIC -shared -Wall $^ -o $@ -lpthread

clean:
	rm -rf $(BUILD) emqx_amd/libtopicmatch.so emqx_amd/libtmwork.so oracle/liboracle.so

.PHONY: all clean

# Erlang NIF shim (needs OTP's erl_nif.h; not present in this image):
#   make nif ERL_INCLUDE=/usr/lib/erlang/usr/include
nif: emqx_amd/libtopicmatch.so
	@test -n "$(ERL_INCLUDE)" || (echo "set ERL_INCLUDE to the directory holding erl_nif.h" && false)
	$(CC) -O2 -fPIC -shared -I$(ERL_INCLUDE) emqx_amd/csrc/emqx_trie_nif.c -Lemqx_amd -ltopicmatch \
	  -Wl,-rpath,'$$ORIGIN' -o emqx_amd/emqx_trie_nif.so
.PHONY: nif

# micro-batcher benchmark (single-topic submits from producer threads)
tools/ubench/batcher_bench: tools/ubench/batcher_bench.cpp emqx_amd/libtopicmatch.so emqx_amd/libtmwork.so include/topicmatch.h
	$(CXX) -O2 -std=c++17 -pthread $< -Lemqx_amd -ltopicmatch -ltmwork -Wl,-rpath,'$$ORIGIN/../../emqx_amd' -o $@

# batcher driver for bench.py's batcher leg (measurement helper, ctypes)
tools/ubench/libbatchdrive.so: tools/ubench/batchdrive.cpp emqx_amd/libtopicmatch.so include/topicmatch.h
	$(CXX) -O2 -std=c++17 -fPIC -shared -pthread $< -Lemqx_amd -ltopicmatch -Wl,-rpath,'$$ORIGIN/../../emqx_amd' -o $@

# deliveries / publish batcher driver of tools/bench_batcher.py --publish (measurement helper, ctypes)
tools/ubench/libpubdrive.so: tools/ubench/pubdrive.cpp emqx_amd/libtopicmatch.so include/topicmatch.h
	$(CXX) -O2 -std=c++17 -fPIC -shared -pthread $< -Lemqx_amd -ltopicmatch -Wl,-rpath,'$$ORIGIN/../../emqx_amd' -o $@

# options batcher flood, host regrouping against the inbox mode (tools/bench_inbox_stream.py; measurement helper, ctypes)
tools/ubench/libinboxdrive.so: tools/ubench/inboxdrive.cpp emqx_amd/libtopicmatch.so include/topicmatch.h
	$(CXX) -O2 -std=c++17 -fPIC -shared -pthread $< -Lemqx_amd -ltopicmatch -Wl,-rpath,'$$ORIGIN/../../emqx_amd' -o $@

# publish batcher flood, host regrouping per node against the forward mode (tools/bench_forward_stream.py; measurement helper, ctypes)
tools/ubench/libfwddrive.so: tools/ubench/fwddrive.cpp emqx_amd/libtopicmatch.so include/topicmatch.h
	$(CXX) -O2 -std=c++17 -fPIC -shared -pthread $< -Lemqx_amd -ltopicmatch -Wl,-rpath,'$$ORIGIN/../../emqx_amd' -o $@

# tm_route_* / tm_sub_* / tm_share_* host calls under AddressSanitizer + UBSan on a host-only engine:
# engine.cpp instrumented, the kernels linked as built and never run.  Leak
# detection stays on for the engine's own allocations; the HIP and RCCL
# runtimes' start-up allocations are suppressed by library name.
SAN = -fsanitize=address,undefined -fno-omit-frame-pointer
SAN_OBJS = $(filter-out $(BUILD)/engine.o,$(filter %.o,$(LIBOBJS)))
san_share: $(LIBOUT)
	$(HIPCC) -O1 -g -fPIC -std=c++17 $(SAN) $(TMDEFS) -c emqx_amd/csrc/engine.cpp -o $(BUILD)/san_engine.o
	$(HIPCC) -O1 -g -fPIC -std=c++17 $(SAN) -c tools/san_share.cpp -o $(BUILD)/san_main.o
	$(HIPCC) --offload-arch=$(ARCH) $(SAN) $(BUILD)/san_main.o $(BUILD)/san_engine.o $(SAN_OBJS) -pthread -L/opt/rocm/lib -lrccl -o $(BUILD)/san_share
	LSAN_OPTIONS=suppressions=tools/san_share.supp $(BUILD)/san_share
.PHONY: san_share

# tm_batcher_* host code (batcher.cpp, publish mode included) and engine.cpp
# under AddressSanitizer + UBSan on a host-only engine: threaded publish
# submits, both mismatched submit kinds, partial takes and a close with
# requests in flight (tools/san_batcher.cpp); the kernels linked as built and
# never run.
SAN_BATCHER_OBJS = $(filter-out $(BUILD)/engine.o $(BUILD)/batcher.o,$(filter %.o,$(LIBOBJS)))
san_batcher: $(LIBOUT)
	$(HIPCC) -O1 -g -fPIC -std=c++17 -Xarch_host -fsanitize=address,undefined -fno-omit-frame-pointer $(TMDEFS) -c emqx_amd/csrc/engine.cpp -o $(BUILD)/san_engine.o
	$(HIPCC) -O1 -g -fPIC -std=c++17 -pthread -Xarch_host -fsanitize=address,undefined -fno-omit-frame-pointer -c emqx_amd/csrc/batcher.cpp -o $(BUILD)/san_batcher_lib.o
	$(HIPCC) -O1 -g -fPIC -std=c++17 -pthread -Xarch_host -fsanitize=address,undefined -fno-omit-frame-pointer -c tools/san_batcher.cpp -o $(BUILD)/san_batcher_main.o
	$(HIPCC) --offload-arch=$(ARCH) $(SAN) $(BUILD)/san_batcher_main.o $(BUILD)/san_engine.o $(BUILD)/san_batcher_lib.o $(SAN_BATCHER_OBJS) -pthread -L/opt/rocm/lib -lrccl -o $(BUILD)/san_batcher
	LSAN_OPTIONS=suppressions=tools/san_share.supp $(BUILD)/san_batcher
.PHONY: san_batcher

# the per-node filters of the host mirror (option "nfilter": relayout with
# extension slots, churn, id reuse, the option switched) under
# AddressSanitizer + UBSan on a host-only engine (tools/san_nfilter.cpp); the
# kernels linked as built and never run.
san_nfilter: $(LIBOUT)
	$(HIPCC) -O1 -g -fPIC -std=c++17 -Xarch_host -fsanitize=address,undefined -fno-omit-frame-pointer $(TMDEFS) -c emqx_amd/csrc/engine.cpp -o $(BUILD)/san_engine.o
	$(HIPCC) -O1 -g -fPIC -std=c++17 -Xarch_host -fsanitize=address,undefined -fno-omit-frame-pointer -c tools/san_nfilter.cpp -o $(BUILD)/san_nfilter_main.o
	$(HIPCC) --offload-arch=$(ARCH) $(SAN) $(BUILD)/san_nfilter_main.o $(BUILD)/san_engine.o $(SAN_OBJS) -pthread -L/opt/rocm/lib -lrccl -o $(BUILD)/san_nfilter
	LSAN_OPTIONS=suppressions=tools/san_share.supp $(BUILD)/san_nfilter
.PHONY: san_nfilter

# the subscription-option host calls (tm_sub_add_opts, tm_sub_set_opts, the
# option pool through growth, in-place rewrites, deletes and compaction, the
# *_opts calls' argument checks) under AddressSanitizer + UBSan on a host-only
# engine (tools/san_subopts.cpp); the kernels linked as built and never run.
san_subopts: $(LIBOUT)
	$(HIPCC) -O1 -g -fPIC -std=c++17 -Xarch_host -fsanitize=address,undefined -fno-omit-frame-pointer $(TMDEFS) -c emqx_amd/csrc/engine.cpp -o $(BUILD)/san_engine.o
	$(HIPCC) -O1 -g -fPIC -std=c++17 -Xarch_host -fsanitize=address,undefined -fno-omit-frame-pointer -c tools/san_subopts.cpp -o $(BUILD)/san_subopts_main.o
	$(HIPCC) --offload-arch=$(ARCH) $(SAN) $(BUILD)/san_subopts_main.o $(BUILD)/san_engine.o $(SAN_OBJS) -pthread -L/opt/rocm/lib -lrccl -o $(BUILD)/san_subopts
	LSAN_OPTIONS=suppressions=tools/san_share.supp $(BUILD)/san_subopts
.PHONY: san_subopts

# the member option pool (the emqx_suboption word of every $share member,
# refreshed by the option calls and the share calls in either order, through
# growth, deletes, member_down and compaction) and the argument checks of the
# pick-word, pack and stream calls with options, under AddressSanitizer + UBSan
# on a host-only engine (tools/san_pickwords.cpp); the kernels linked as built
# and never run.
san_pickwords: $(LIBOUT)
	$(HIPCC) -O1 -g -fPIC -std=c++17 -Xarch_host -fsanitize=address,undefined -fno-omit-frame-pointer $(TMDEFS) -c emqx_amd/csrc/engine.cpp -o $(BUILD)/san_engine.o
	$(HIPCC) -O1 -g -fPIC -std=c++17 -Xarch_host -fsanitize=address,undefined -fno-omit-frame-pointer -c tools/san_pickwords.cpp -o $(BUILD)/san_pickwords_main.o
	$(HIPCC) --offload-arch=$(ARCH) $(SAN) $(BUILD)/san_pickwords_main.o $(BUILD)/san_engine.o $(SAN_OBJS) -pthread -L/opt/rocm/lib -lrccl -o $(BUILD)/san_pickwords
	LSAN_OPTIONS=suppressions=tools/san_share.supp $(BUILD)/san_pickwords
.PHONY: san_pickwords

# the micro-batcher's admission mode (TM_BATCHER_ADMIT: the open and submit
# checks, the credential records through threaded submits, partial takes,
# both plans and a close with requests in flight) and the host admission
# forms of admit.hip, under AddressSanitizer + UBSan on a host-only engine
# (tools/san_admit.cpp); the kernels linked as built and never run.
SAN_ADMIT_OBJS = $(filter-out $(BUILD)/engine.o $(BUILD)/batcher.o $(BUILD)/admit.o,$(filter %.o,$(LIBOBJS)))
san_admit: $(LIBOUT)
	$(HIPCC) -O1 -g -fPIC -std=c++17 -Xarch_host -fsanitize=address,undefined -fno-omit-frame-pointer $(TMDEFS) -c emqx_amd/csrc/engine.cpp -o $(BUILD)/san_engine.o
	$(HIPCC) -O1 -g -fPIC -std=c++17 -pthread -Xarch_host -fsanitize=address,undefined -fno-omit-frame-pointer -c emqx_amd/csrc/batcher.cpp -o $(BUILD)/san_batcher_lib.o
	$(HIPCC) --offload-arch=$(ARCH) -O1 -g -fPIC -std=c++17 -Xarch_host -fsanitize=address,undefined -fno-omit-frame-pointer -c emqx_amd/csrc/admit.hip -o $(BUILD)/san_admit_lib.o
	$(HIPCC) -O1 -g -fPIC -std=c++17 -pthread -Xarch_host -fsanitize=address,undefined -fno-omit-frame-pointer -c tools/san_admit.cpp -o $(BUILD)/san_admit_main.o
	$(HIPCC) --offload-arch=$(ARCH) $(SAN) $(BUILD)/san_admit_main.o $(BUILD)/san_engine.o $(BUILD)/san_batcher_lib.o $(BUILD)/san_admit_lib.o $(SAN_ADMIT_OBJS) -pthread -L/opt/rocm/lib -lrccl -o $(BUILD)/san_admit
	LSAN_OPTIONS=suppressions=tools/san_share.supp $(BUILD)/san_admit
.PHONY: san_admit
