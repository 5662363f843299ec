#!/bin/bash
# Timeline of one k_step_patch launch (IPP_TIMELINE build), each step under its own timeout.
cd "$GRAFT_REPO_ROOT"; O=gpurun_out/ab; mkdir -p $O
{
  IPP_TIMELINE_FILE=$O/tl.bin timeout 300 python tools/ab_kernels.py --window-rows 10 --rounds 20 --order desc t=tools/probes/libipp_timing.so 2>&1 | grep -v amdgpu.ids | tail -2
  timeout 60 python tools/timeline.py $O/tl.bin 4096 10
} 2>&1 | tee $O/timeline.txt
rm -f $O/*.bin
