# Builds the product library (HIP, gfx950 only) and the CPU oracle (tests only).
#   make            -> vettore_amd/lib/libvettore_hip.so + oracle/libvt_oracle.so (+ the tests' own libraries)
# hipcc cross-compiles for gfx950 without a GPU present.
ROCM    ?= /opt/rocm
HIPCC   ?= $(ROCM)/bin/hipcc
ARCH    ?= gfx950
CSRC    := vettore_amd/csrc
LIBDIR  := vettore_amd/lib
# -ffp-contract=off: the reference never fuses a*b+c; the kernels must not either.
HIPFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -ffp-contract=off \
            -fhip-fp32-correctly-rounded-divide-sqrt -Wall -Wno-unused-function

# `make experiments`: the same library with the timing experiments of K2 / K2b / K2s / K1m compiled in and their
# settings named (batch_debug, mq_dbg, shadow_stages, trace_batch: csrc/vt_env.h) -> vettore_amd/lib/experiments/
# libvettore_hip.so.  Wrong results on purpose (barriers removed, stages skipped): for the cost breakdowns in
# DESIGN_APPENDIX only, never loaded by a test.  The product build carries neither the switches nor the code behind them.
# Kernels that must not spill are checked after they are compiled (tools/check_scratch.py says why); the experiments' extra
# registers do spill, and nobody ships that build.
CHECK_SCRATCH := python3 tools/check_scratch.py
ifdef EXPERIMENTS
HIPFLAGS += -DVT_EXPERIMENTS -DVT_BATCH_TIMING_EXPERIMENTS -DVT_MULTI_TIMING_EXPERIMENTS
CHECK_SCRATCH := @true
endif

# (vt_scan_multi first: alone it compiles for as long as all the others together at -j4, so a clean build lasts as long
# as that unit does once it starts at once; vt_hamming is the next longest at half of it)
DEVSRC  := vt_scan_multi vt_select vt_hamming vt_ingest vt_cosine vt_scan vt_batch vt_batch_bf16 vt_batch_shadow vt_scan_dot vt_scan_l2 vt_scan_l1 vt_scan_misc vt_scan_general vt_scan_gather vt_scan_filter vt_prefix_multi vt_maxsim vt_maxsim_resident vt_maxsim_batch vt_muvera vt_sketch vt_sketch_batch vt_sketch_nibble vt_sketch4_rescore vt_hnsw vt_hnsw_stage vt_mmr vt_prepare
DEVOBJ  := $(addprefix $(LIBDIR)/,$(addsuffix .o,$(DEVSRC)))
DEVHDR  := $(CSRC)/vt_device.h $(CSRC)/vt_common.cuh $(CSRC)/vt_scan.cuh $(CSRC)/vt_env.h

all: $(LIBDIR)/libvettore_hip.so $(LIBDIR)/libvettore_hip_hooks.so $(LIBDIR)/libvt_callers.so $(LIBDIR)/libvt_callers_hooks.so $(LIBDIR)/libvt_sketch_probe.so $(LIBDIR)/libvt_sketch4_probe.so $(LIBDIR)/libvt_sketch4_finish_probe.so $(LIBDIR)/libvt_sketch4_rescore_probe.so $(LIBDIR)/libvt_sketch4_best_probe.so $(LIBDIR)/libvt_sketch_l2_probe.so $(LIBDIR)/libvt_sketch_batch_probe.so $(LIBDIR)/libvt_batch_probe.so $(LIBDIR)/libvt_hnsw_compact_probe.so $(LIBDIR)/libvt_panel_probe.so $(LIBDIR)/libvt_select_probe.so $(LIBDIR)/libvt_hnsw_stage_probe.so oracle

# What a device unit's build checks or adds, per unit:
#   NOSCRATCH_<unit>  kernels that must neither spill nor carry a scratch segment
#   NOSPILL_<unit>    kernels that must not spill (tools/check_scratch.py says why): the build fails if one does
#   EXTRA_<unit>      compiler flags of that unit alone
# K1's instantiation units: no scratch at all (r05: the overflow recovery returns its value by value; every launch of a
# kernel with a scratch segment has it set up)
K1_UNITS := vt_scan_dot vt_scan_l2 vt_scan_l1 vt_scan_misc vt_scan_general vt_scan_gather vt_scan_filter
$(foreach u,$(K1_UNITS),$(eval NOSCRATCH_$(u) := scan_topk_kernel))
NOSCRATCH_vt_scan_multi   := scan_multi_kernel
NOSCRATCH_vt_prefix_multi := prefix_multi_kernel
# (-fno-slp-vectorize: K1p packs two ELEMENTS of a query per instruction by hand; the SLP pass re-packs two QUERIES
# instead, with a register move per operand pair -- 22-26 % more VALU cycles per chunk, measured)
EXTRA_vt_prefix_multi     := -fno-slp-vectorize
# K9 (MaxSim): the overflow recovery returns by value, as in K1 -- no scratch segment behind any launch
NOSCRATCH_vt_maxsim       := maxsim_kernel
# K9r (MaxSim over a resident store): K9's arithmetic and its recovery by value -- no scratch segment either
NOSCRATCH_vt_maxsim_resident := maxsim_resident_kernel
# K9rb (K9r over many query sets): the same pass (vt_maxsim_pair.cuh), the sets' totals in registers -- no scratch segment
NOSCRATCH_vt_maxsim_batch := maxsim_batch_kernel
# K10 (MUVERA): one lane's f64 chain per dot product, nothing indexed dynamically in registers
NOSCRATCH_vt_muvera       := muvera_encode_kernel muvera_encode_slab_kernel muvera_sketch_kernel muvera_table_kernel
# K1q, K1s, K1f and K1n (the int8, 6-bit, 5-bit and 4-bit sketch passes): the register ring must stay in registers; K1q's
# tail and the threshold, refine and collect kernels behind the other three likewise carry no scratch segment
NOSCRATCH_vt_sketch       := sketch_scan_kernel sketch_tail_kernel sketch_tail_group_kernel sketch_thresh_kernel sketch_refine_kernel sketch_collect_kernel
# K1qm (a group of 2..8 queries in one pass over the int8 sketch): 2 G sums per lane beside the ring, all in registers
NOSCRATCH_vt_sketch_batch := sketch_scan_multi_kernel
NOSCRATCH_vt_sketch_nibble := sketch6_scan_kernel sketch5_scan_kernel sketch4_scan_kernel
# The nibble passes (K1s, K1f, K1n: one skeleton, vt_sketch_nibble.cuh) branch three ways per run on wave-uniform cursors --
# H-run, L-run, metadata; K1n two ways.  By default the CFG structurizer lays the three arms out in
# a row behind flags, as it must for divergent branches, and every sum then lives across all arms and is copied in each
# (about 400 v_mov_b32 per tile at d = 768, profiles/sketch6_loop/isa_counts.txt); told to leave wave-uniform regions as
# written, the arms hold their dots alone.  For that unit only: no other kernel is built this way.
# The option is an internal one of LLVM, off by default: the figures (85 VGPRs, 5 waves / SIMD, 648 VALU instructions in a
# tile's run blocks) are this toolchain's.  A compiler without it fails the build (unknown argument); one that changes what
# it does still builds a correct kernel (every test holds either way) but may bring the copies back: after a ROCm update
# count again as profiles/sketch6_loop/isa_counts.txt says, and compare the pass's time.
# (The three widths' builders are in the unit too.  K1s's were built without the option before they moved here and come out
# instruction for instruction as they did: profiles/sketch_nibble/isa_counts.txt.)
EXTRA_vt_sketch_nibble    := -mllvm -structurizecfg-skip-uniform-regions=true
# K1n's last link (candidates rescored from the pass's lists): a round of loaded rows indexed statically, the recovery by
# value as in K1 -- no scratch segment, no spill
NOSCRATCH_vt_sketch4_rescore := sketch4_rescore_kernel
# K11 (HNSW traversals): the distance chains are K9's with the recovery by value; heaps and visited set live in the
# slot's global scratch, nothing is indexed dynamically in registers -- no scratch segment
NOSCRATCH_vt_hnsw         := hnsw_traverse_kernel
# K15 (the staged searches' scores over an HNSW slab): K11's chains, one lane a pair, the recovery by value; the sign-bit
# sweep keeps its counts in scalar registers -- no scratch segment
NOSCRATCH_vt_hnsw_stage   := hnsw_stage_bits_kernel hnsw_stage_score_kernel
# K12 (MMR steps): one lane's chain per pair, K9's, with the recovery by value -- no scratch segment behind any of a call's launches
NOSCRATCH_vt_mmr          := mmr_step_kernel
# K14 (prepare rows): a lane's chain accumulators and a batch of loaded runs, all indexed statically -- no scratch segment
NOSCRATCH_vt_prepare      := prepare_rows_kernel
NOSPILL_vt_batch_bf16     := bf16_scores_kernel
NOSPILL_vt_batch_shadow   := shadow_scores_kernel

# (the compiler's remarks, and with them its warnings and errors, go to <unit>.resources: shown when the compile fails)
$(LIBDIR)/%.o: $(CSRC)/%.hip $(DEVHDR)
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) $(EXTRA_$*) -Rpass-analysis=kernel-resource-usage -c $< -o $@ 2> $(LIBDIR)/$*.resources || { grep -v 'remark:' $(LIBDIR)/$*.resources >&2; exit 1; }
	$(if $(NOSCRATCH_$*),$(CHECK_SCRATCH) --no-scratch $(LIBDIR)/$*.resources $(NOSCRATCH_$*))
	$(if $(NOSPILL_$*),$(CHECK_SCRATCH) $(LIBDIR)/$*.resources $(NOSPILL_$*))

# (what the sketch units share)
$(LIBDIR)/vt_sketch.o $(LIBDIR)/vt_sketch_batch.o $(LIBDIR)/vt_sketch_nibble.o: $(CSRC)/vt_sketch.cuh
$(LIBDIR)/vt_sketch_nibble.o: $(CSRC)/vt_sketch_nibble.cuh
# (one row's exact key by one wave: the refine kernel and the 4-bit pass's best rows)
$(LIBDIR)/vt_sketch.o $(LIBDIR)/vt_sketch_nibble.o: $(CSRC)/vt_rowscore.cuh
$(LIBDIR)/vt_sketch_batch.o: $(CSRC)/host/vt_sketchbatch.h

# (the one-lane pair arithmetic of K9, K9r, K9rb, K11, K12 and K15p; what the three MaxSim kernels share beside it)
$(LIBDIR)/vt_maxsim.o $(LIBDIR)/vt_maxsim_resident.o $(LIBDIR)/vt_maxsim_batch.o $(LIBDIR)/vt_hnsw.o $(LIBDIR)/vt_hnsw_stage.o $(LIBDIR)/vt_mmr.o: $(CSRC)/vt_pair.cuh
$(LIBDIR)/vt_maxsim.o $(LIBDIR)/vt_maxsim_resident.o $(LIBDIR)/vt_maxsim_batch.o: $(CSRC)/vt_maxsim_pair.cuh

# (the row-panel walk of K6b, K6bm and K1p and the group epilogue of the latter two)
$(LIBDIR)/vt_cosine.o $(LIBDIR)/vt_prefix_multi.o: $(CSRC)/vt_panel.cuh

# (what the matrix-core nomination passes K2, K2b and K2s share: DMA piece, tile sequence and cursor, epilogue, launch)
$(LIBDIR)/vt_batch.o $(LIBDIR)/vt_batch_bf16.o $(LIBDIR)/vt_batch_shadow.o: $(CSRC)/vt_nominate.cuh

HOSTHDR := $(wildcard $(CSRC)/host/*.h)
$(LIBDIR)/vt_index.o: $(CSRC)/vt_index.cpp $(HOSTHDR) $(CSRC)/vt_device.h $(CSRC)/vt_env.h include/vettore_flat.h
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -x hip -c $< -o $@

# (only the C ABI is exported: csrc/exports.map)
EXPORTS := -Wl,--version-script=$(CSRC)/exports.map
$(LIBDIR)/libvettore_hip.so: $(DEVOBJ) $(LIBDIR)/vt_index.o $(CSRC)/exports.map
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(filter %.o,$^) $(EXPORTS) -lpthread -ldl

# The same library with the fault-injection hooks compiled into the host side (VT_TEST_FAIL_AFTER_ID_UPDATE,
# VT_TEST_FOREIGN_ROWS): test infrastructure, loaded only by the two tests that need them
# (VETTORE_HIP_LIB=...); the product library carries no such switch.
$(LIBDIR)/vt_index_hooks.o: $(CSRC)/vt_index.cpp $(HOSTHDR) $(CSRC)/vt_device.h $(CSRC)/vt_env.h include/vettore_flat.h
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -DVT_TEST_HOOKS -x hip -c $< -o $@

$(LIBDIR)/libvettore_hip_hooks.so: $(DEVOBJ) $(LIBDIR)/vt_index_hooks.o $(CSRC)/exports.map
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(filter %.o,$^) $(EXPORTS) -lpthread -ldl

experiments:
	$(MAKE) EXPERIMENTS=1 LIBDIR=vettore_amd/lib/experiments vettore_amd/lib/experiments/libvettore_hip.so

# bench.py's native caller threads (tools/callers_native.cpp): measurement infrastructure, not product
$(LIBDIR)/libvt_callers.so: tools/callers_native.cpp include/vettore_flat.h $(LIBDIR)/libvettore_hip.so
	g++ -O2 -std=c++17 -fPIC -shared tools/callers_native.cpp -Iinclude -L$(LIBDIR) -lvettore_hip -lpthread -Wl,-rpath,'$$ORIGIN' -o $@

# the same callers bound to the hooks build (tests that force callers to meet: vt_callers_meet with `hold`)
$(LIBDIR)/libvt_callers_hooks.so: tools/callers_native.cpp include/vettore_flat.h $(LIBDIR)/libvettore_hip_hooks.so
	g++ -O2 -std=c++17 -fPIC -shared tools/callers_native.cpp -Iinclude -L$(LIBDIR) -lvettore_hip_hooks -lpthread -Wl,-rpath,'$$ORIGIN' -o $@

# The sketch kernels on their own behind a probe (tests/sketch_probe.cpp: the four builders and passes and the spread certification
# launched one at a time on a test's arrays; tests/test_gpu_sketch_kernels.py loads it with ctypes): test infrastructure.
# vt_sketch.o, vt_sketch_nibble.o and the probe, nothing else of the library, and no export map; the package never loads it.
$(LIBDIR)/sketch_probe.o: tests/sketch_probe.cpp $(CSRC)/vt_device.h $(CSRC)/host/vt_sketch5.h $(CSRC)/host/vt_sketch6.h
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -I$(CSRC) -x hip -c $< -o $@

$(LIBDIR)/libvt_sketch_probe.so: $(LIBDIR)/vt_sketch.o $(LIBDIR)/vt_sketch_nibble.o $(LIBDIR)/sketch_probe.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -Wl,--no-undefined -o $@ $^

# K1n's kernels behind a probe of their own (tests/sketch4_probe.cpp; tests/test_gpu_sketch4_kernels.py loads it): the
# builders, the pass, and the threshold, refine and collect launches on a test's arrays.  Test infrastructure, as above.
$(LIBDIR)/sketch4_probe.o: tests/sketch4_probe.cpp $(CSRC)/vt_device.h
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -I$(CSRC) -x hip -c $< -o $@

$(LIBDIR)/libvt_sketch4_probe.so: $(LIBDIR)/vt_sketch.o $(LIBDIR)/vt_sketch_nibble.o $(LIBDIR)/sketch4_probe.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -Wl,--no-undefined -o $@ $^

# The kernel that finishes K1n's chain behind a probe (tests/sketch4_finish_probe.cpp; tests/test_gpu_sketch4_finish_kernels.py
# loads it): the gathered K1 in filter mode on a test's arrays.  Test infrastructure, as above.
$(LIBDIR)/sketch4_finish_probe.o: tests/sketch4_finish_probe.cpp $(CSRC)/vt_device.h
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -I$(CSRC) -x hip -c $< -o $@

$(LIBDIR)/libvt_sketch4_finish_probe.so: $(LIBDIR)/vt_scan_filter.o $(LIBDIR)/sketch4_finish_probe.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -Wl,--no-undefined -o $@ $^

# K1n's last link behind a probe (tests/sketch4_rescore_probe.cpp; tests/test_gpu_sketch4_rescore_kernels.py loads it): the
# rescoring kernel on a test's hand-made lists.  Test infrastructure, as above.
$(LIBDIR)/sketch4_rescore_probe.o: tests/sketch4_rescore_probe.cpp $(CSRC)/vt_device.h
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -I$(CSRC) -x hip -c $< -o $@

$(LIBDIR)/libvt_sketch4_rescore_probe.so: $(LIBDIR)/vt_sketch4_rescore.o $(LIBDIR)/sketch4_rescore_probe.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -Wl,--no-undefined -o $@ $^

# K1n's threshold from its lists' best rows behind a probe (tests/sketch4_best_probe.cpp; tests/test_gpu_sketch4_best_kernels.py
# loads it): the 4-bit pass asked for the best words, and the rescoring kernel handed such words.  Test infrastructure, as above.
$(LIBDIR)/sketch4_best_probe.o: tests/sketch4_best_probe.cpp $(CSRC)/vt_device.h
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -I$(CSRC) -x hip -c $< -o $@

$(LIBDIR)/libvt_sketch4_best_probe.so: $(LIBDIR)/vt_sketch_nibble.o $(LIBDIR)/vt_sketch4_rescore.o $(LIBDIR)/sketch4_best_probe.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -Wl,--no-undefined -o $@ $^

# The int8 sketch's L2 family behind a probe (tests/sketch_l2_probe.cpp; tests/test_gpu_sketch_l2_kernels.py loads it): the
# builders with and without xx, the pass in either metric family and the one-block tail on a test's arrays.  vt_sketch.o and
# the probe, nothing else of the library.  Test infrastructure, as above.
$(LIBDIR)/sketch_l2_probe.o: tests/sketch_l2_probe.cpp $(CSRC)/vt_device.h
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -I$(CSRC) -x hip -c $< -o $@

$(LIBDIR)/libvt_sketch_l2_probe.so: $(LIBDIR)/vt_sketch.o $(LIBDIR)/sketch_l2_probe.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -Wl,--no-undefined -o $@ $^

# K1qm's kernels behind a probe (tests/sketch_batch_probe.cpp; tests/test_gpu_sketch_batch_kernels.py loads it): the group
# pass and the group tail beside the lone pass and the lone tail, on a test's arrays.  Test infrastructure, as above.
$(LIBDIR)/sketch_batch_probe.o: tests/sketch_batch_probe.cpp $(CSRC)/vt_device.h
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -I$(CSRC) -x hip -c $< -o $@

$(LIBDIR)/libvt_sketch_batch_probe.so: $(LIBDIR)/vt_sketch.o $(LIBDIR)/vt_sketch_batch.o $(LIBDIR)/sketch_batch_probe.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -Wl,--no-undefined -o $@ $^

# The matrix-core nomination kernels behind a probe (tests/batch_probe.cpp; tests/test_gpu_batch_kernels.py loads it): K2, K2b
# and K2s in pass and dense mode, the images, the row norms, the threshold kernels and the batched select on a test's arrays,
# with the certificate's margin (host/vt_batchbound.h) exported beside them.  vt_batch.o, vt_batch_bf16.o, vt_batch_shadow.o
# and the probe, nothing else of the library.  Test infrastructure, as above.
$(LIBDIR)/batch_probe.o: tests/batch_probe.cpp $(CSRC)/vt_device.h $(CSRC)/vt_env.h $(CSRC)/host/vt_batchbound.h
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -I$(CSRC) -x hip -c $< -o $@

$(LIBDIR)/libvt_batch_probe.so: $(LIBDIR)/vt_batch.o $(LIBDIR)/vt_batch_bf16.o $(LIBDIR)/vt_batch_shadow.o $(LIBDIR)/batch_probe.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -Wl,--no-undefined -o $@ $^

# K11c behind a probe (tests/hnsw_compact_probe.cpp; tests/test_gpu_hnsw_compact_kernel.py loads it): the compaction of an
# HNSW slab and its mirror on a test's hand-made arrays, and its timing beside a plain copy.  vt_hnsw.o and the probe,
# nothing else of the library.  Test infrastructure, as above.
$(LIBDIR)/hnsw_compact_probe.o: tests/hnsw_compact_probe.cpp $(CSRC)/vt_device.h
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -I$(CSRC) -x hip -c $< -o $@

$(LIBDIR)/libvt_hnsw_compact_probe.so: $(LIBDIR)/vt_hnsw.o $(LIBDIR)/hnsw_compact_probe.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -Wl,--no-undefined -o $@ $^

# The row-panel kernels behind a probe (tests/panel_probe.cpp; tests/test_gpu_panel_kernels.py loads it): K1p, K6bm and K6b
# launched one at a time on a test's arrays -- sample cells, tile maxima, lists, counts and the status word read back.
# vt_cosine.o, vt_prefix_multi.o and the probe, nothing else of the library.  Test infrastructure, as above.
$(LIBDIR)/panel_probe.o: tests/panel_probe.cpp $(CSRC)/vt_device.h $(CSRC)/vt_env.h
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -I$(CSRC) -x hip -c $< -o $@

$(LIBDIR)/libvt_panel_probe.so: $(LIBDIR)/vt_cosine.o $(LIBDIR)/vt_prefix_multi.o $(LIBDIR)/panel_probe.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -Wl,--no-undefined -o $@ $^

# The selection kernels behind a probe (tests/select_probe.cpp; tests/test_gpu_select_kernels.py loads it): K3's one-block
# radix select in its five launch forms, the spread select, the list sort, the cross-shard merge and the radix k-th passes
# with their collect, launched one at a time on a test's arrays -- whole result blocks, lists, counts and the status word
# read back.  vt_select.o and the probe, nothing else of the library.  Test infrastructure, as above.
$(LIBDIR)/select_probe.o: tests/select_probe.cpp $(CSRC)/vt_device.h
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -I$(CSRC) -x hip -c $< -o $@

$(LIBDIR)/libvt_select_probe.so: $(LIBDIR)/vt_select.o $(LIBDIR)/select_probe.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -Wl,--no-undefined -o $@ $^

# K15 behind a probe (tests/hnsw_stage_probe.cpp; tests/test_gpu_hnsw_stage_kernels.py loads it): the sign-bit sweep and
# the prefix scores over a test's hand-made slab, every key and payload of the column read back.  vt_hnsw_stage.o and the
# probe, nothing else of the library.  Test infrastructure, as above.
$(LIBDIR)/hnsw_stage_probe.o: tests/hnsw_stage_probe.cpp $(CSRC)/vt_device.h
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -I$(CSRC) -x hip -c $< -o $@

$(LIBDIR)/libvt_hnsw_stage_probe.so: $(LIBDIR)/vt_hnsw_stage.o $(LIBDIR)/hnsw_stage_probe.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -Wl,--no-undefined -o $@ $^

oracle:
	$(MAKE) -C oracle -s

# stand-alone hardware probes quoted in DESIGN.md (not part of the library)
PROBES := tools/hbm_peak tools/launch_probe tools/mfma_peak tools/mfma_agpr tools/vmm_probe
probes: $(PROBES)
tools/%: tools/%.hip
	$(HIPCC) --offload-arch=$(ARCH) -O3 $< -o $@

clean:
	rm -rf $(LIBDIR) oracle/libvt_oracle.so $(PROBES)

.PHONY: all oracle clean probes experiments
