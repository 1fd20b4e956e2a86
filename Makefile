# Build of the MI355X likelihood engine (gfx950 only), its host mirror and the CPU oracle.
#   make            -> everything that ships to the GPU box
#   make ref        -> oracle/_ref (needs /root/reference; container only)
HIPCC      ?= /opt/rocm/bin/hipcc
CXX        ?= g++
CC         ?= gcc
ARCH       := gfx950
PKG        := iq-tree_amd
CSRC       := $(PKG)/csrc
HOST       := $(PKG)/host
LIBDIR     := $(PKG)/lib
HIPFLAGS   := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -Wno-unused-value -Wno-unused-result
HIP_SRCS   := $(CSRC)/engine.hip $(CSRC)/solve.hip $(CSRC)/plan.hip $(CSRC)/ptnlh.hip $(CSRC)/ufboot.hip $(CSRC)/classlh.hip $(CSRC)/pairdist.hip $(CSRC)/quartet.hip $(CSRC)/kernels_valu4.hip $(CSRC)/kernels_valu4w.hip $(CSRC)/kernels_mfma.hip $(CSRC)/kernels_newton.hip $(CSRC)/kernels_partnewton.hip $(CSRC)/kernels_partboot.hip $(CSRC)/kernels_partdist.hip $(CSRC)/partition.hip $(CSRC)/kernels_sweep.hip $(CSRC)/kernels_rell.hip $(CSRC)/kernels_em.hip $(CSRC)/kernels_mixem.hip $(CSRC)/kernels_classlnl.hip $(CSRC)/kernels_alrt.hip $(CSRC)/kernels_topo.hip $(CSRC)/kernels_ufboot.hip $(CSRC)/kernels_dist.hip $(CSRC)/kernels_quartet.hip $(CSRC)/kernels_bionj.hip $(CSRC)/kernels_pars.hip $(CSRC)/kernels_spr.hip $(CSRC)/pars.hip $(CSRC)/comm.hip $(CSRC)/sharded.hip
HIP_OBJS   := $(patsubst $(CSRC)/%.hip,$(LIBDIR)/%.o,$(HIP_SRCS))

all: $(LIBDIR)/libiqhip.so $(LIBDIR)/libiqhost.so $(LIBDIR)/iqhip_lnl oracle/liblh_oracle.so

$(LIBDIR):
	mkdir -p $(LIBDIR)

$(LIBDIR)/%.o: $(CSRC)/%.hip $(CSRC)/iqhip_internal.h $(CSRC)/wg_exchange.h $(CSRC)/trav_lds.h $(CSRC)/trav_phases.h $(CSRC)/pars_spr_check.h $(CSRC)/ufboot_rule.h $(CSRC)/pair_eval.h $(CSRC)/partpair_layout.h $(CSRC)/partition.h include/iqhip.h | $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# the topology tests compare sums bit for bit with a plain IEEE evaluation of the reference's expressions
$(LIBDIR)/kernels_topo.o: HIPFLAGS += -ffp-contract=off
# ... and so does the UFBoot bookkeeping with its numpy restatement
$(LIBDIR)/kernels_ufboot.o: HIPFLAGS += -ffp-contract=off
$(LIBDIR)/kernels_partboot.o: HIPFLAGS += -ffp-contract=off
# ... and the pairwise distances follow a numpy restatement step for step
$(LIBDIR)/kernels_dist.o: HIPFLAGS += -ffp-contract=off
$(LIBDIR)/kernels_partdist.o: HIPFLAGS += -ffp-contract=off
# ... and the quartet likelihoods of likelihood mapping likewise
$(LIBDIR)/kernels_quartet.o: HIPFLAGS += -ffp-contract=off
$(LIBDIR)/quartet.o: HIPFLAGS += -ffp-contract=off
# ... and so does BIONJ
$(LIBDIR)/kernels_bionj.o: HIPFLAGS += -ffp-contract=off

$(LIBDIR)/libiqhip.so: $(HIP_OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(HIP_OBJS) -ldl

HOST_SRCS  := $(HOST)/phylo_host.cpp $(HOST)/phylo_nni.cpp $(HOST)/phylo_support.cpp $(HOST)/phylo_dist.cpp $(HOST)/phylo_pars.cpp $(HOST)/phylo_em.cpp $(HOST)/phylo_ufboot.cpp $(HOST)/iqhost_c.cpp $(HOST)/model_host.cpp $(HOST)/alignment_host.cpp $(HOST)/iqmodel_c.cpp $(HOST)/model_opt_host.cpp $(HOST)/supertree_host.cpp $(HOST)/tree_search_host.cpp $(HOST)/pars_forest_host.cpp
HOST_HDRS  := $(HOST)/search_host.h $(HOST)/tree_search_host.h $(HOST)/pars_forest_host.h $(HOST)/pars_forest_plan.h $(HOST)/phylo_host.h $(HOST)/mirror_policy.h $(HOST)/brent_host.h $(HOST)/bfgs_host.h $(HOST)/model_host.h $(HOST)/model_opt_host.h $(HOST)/alignment_host.h $(HOST)/ufboot_splits.h $(HOST)/supertree_host.h $(HOST)/supertree_brlen.h $(HOST)/partition_spec.h $(HOST)/lmap_host.h include/iqhip.h include/iqhip_adapter.h

$(LIBDIR)/libiqhost.so: $(HOST_SRCS) $(HOST_HDRS) $(LIBDIR)/libiqhip.so
	$(CXX) -O2 -std=c++17 -fPIC -shared -Wall -o $@ $(HOST_SRCS) -L$(LIBDIR) -liqhip -Wl,-rpath,'$$ORIGIN'

# stand-alone driver (the reference's "-s -te -m -blfix -n 0" evaluation) on top of the same libraries
$(LIBDIR)/iqhip_lnl: cli/iqhip_lnl.cpp $(HOST_HDRS) $(LIBDIR)/libiqhost.so
	$(CXX) -O2 -std=c++17 -Wall -o $@ cli/iqhip_lnl.cpp -L$(LIBDIR) -liqhost -liqhip -Wl,-rpath,'$$ORIGIN'

oracle/liblh_oracle.so: oracle/lh_oracle.c
	$(CC) -O3 -mavx -fopenmp -ffp-contract=off -fPIC -shared -Wall -Wextra -o $@ $< -lm

ref:
	$(MAKE) -C oracle ref

clean:
	rm -rf $(LIBDIR) oracle/liblh_oracle.so oracle/_ref

.PHONY: all ref clean
