#!/bin/bash
# VGPRs / scratch / LDS of every kernel of the seventeen kernel units, each with the flags the Makefile builds it with (no GPU needed).
cd "$(dirname "$0")/../jefferson-2.0_amd/csrc"
# unit : the Makefile's flags beside CXXFLAGS (KERNEL_FLAGS, and KFLAGS where `make variant` passes it)
for unit in "jf_kernels.hip:-fno-slp-vectorize $KFLAGS" "jf_reverb.hip:-fno-slp-vectorize $KFLAGS" "jf_kernels2048.hip:-fno-slp-vectorize" \
            "jf_room.hip:-fno-slp-vectorize" "jf_live.hip:" "jf_pose.hip:-ffp-contract=off" "jf_desc_edit.hip:-ffp-contract=off" \
            "jf_master.hip:-ffp-contract=off" "jf_lookahead.hip:-ffp-contract=off" "jf_gate.hip:-ffp-contract=off" "jf_voice.hip:-ffp-contract=off" "jf_level.hip:-ffp-contract=off" "jf_range.hip:-ffp-contract=off" "jf_cone.hip:-ffp-contract=off" "jf_follow.hip:-ffp-contract=off" "jf_stream.hip:-ffp-contract=off" "jf_output.hip:-ffp-contract=off"; do
  f=${unit%%:*}
  echo "== $f"
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC ${unit#*:} -S --cuda-device-only -o /dev/null $f \
      -Rpass-analysis=kernel-resource-usage 2>&1 |
  sed 's/ \[-Rpass-analysis=kernel-resource-usage\]//' |
  awk '/Function Name:/ {n=$NF} /remark: +VGPRs:/ {v=$NF} /ScratchSize/ {s=$NF} /LDS Size/ {print n, "vgpr", v, "scratch", s, "lds", $NF}' | c++filt
done
