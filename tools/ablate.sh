#!/bin/bash
# developer tool: builds variants of libpbrs_gpu.so for in-session A/B timing: tools/ablate.sh name:flags ...
# (the Makefile's `gpu` target under another name, pbrs_amd/lib/abl_<name>.so, every unit with the extra flags: they reach the host-only
# upload steps too, which read PBRS_FLAT_TLAS_MAX*, PBRS_WIDE_* and PBRS_REFILL_BELOW_*)
cd "$(dirname "$0")/../pbrs_amd/csrc" || exit 1
for v in "$@"; do
  name=${v%%:*}; flags=${v#*:}
  make gpu NAME=abl_$name HIPCC_EXTRA="$flags -Rpass-analysis=kernel-resource-usage" > /tmp/abl_$name.log 2>&1 &
done
wait
for v in "$@"; do name=${v%%:*}; echo "== $name"; grep -E "Function Name|VGPRs:|ScratchSize" /tmp/abl_$name.log | sed 's/.*remark: //; s/ \[-Rpass.*//' | paste - - - | grep -E "shade|extendILb0|shadowILb0" | sed 's/Function Name: //'; done
