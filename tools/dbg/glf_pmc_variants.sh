#!/bin/bash
# usage (GPU box): bash tools/dbg/glf_pmc_variants.sh "<name>:<flags>" ...  -- SQ counters (tools/pmc_step.sh, 8192-site tile) of the SNP step with glfgen.hip
# built with other options; the variant library is built outside the tree and loaded through BCFGPU_SO.  Prints the counters of
# glfgen_kernel per variant, then the other kernels of the step as the first variant's run measured them.
R=$GRAFT_REPO_ROOT
ALL="glfgen combine mcall indel gap_prep baq overlap pileup gvcf gather capmapq draw api tables"
PROD=$(make -s -C $R/bcftools_amd/csrc print-flags-glfgen)
OBJS=""; for o in $ALL; do if [ "$o" = glfgen ]; then OBJS="$OBJS /tmp/gpv.o"; else OBJS="$OBJS $R/bcftools_amd/csrc/$o.o"; fi; done
others=
for spec in "$@"; do
  name=${spec%%:*}; flags="$PROD ${spec#*:}"
  cd $R/bcftools_amd/csrc
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wno-unused-value $flags -c glfgen.hip -o /tmp/gpv.o 2>/dev/null || { echo "$name: build failed"; continue; }
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o /tmp/gpv.so $OBJS -ldl
  res=$(BCFGPU_SO=/tmp/gpv.so bash $R/tools/pmc_step.sh gpv_$name 2>/dev/null)     # (pmc_step.sh ends by printing its counters)
  echo "== $name ($flags)"
  grep "glfgen_kernel<false, true, false>" <<< "$res"
  [ -n "$others" ] || others=$(grep -v glfgen <<< "$res")
done
echo "== the other kernels of the step"
echo "$others"
