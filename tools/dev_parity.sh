#!/bin/bash
# developer tool (GPU box): the whole GPU parity suite through a developer build under developer overrides
# (pbrs_amd/lib/abl_<name>.so built with -DPBRS_DEV_OVERRIDES: tools/ablate.sh "dev:-DPBRS_DEV_OVERRIDES"), one run per setting.
#   usage: tools/dev_parity.sh dev "PBRS_WIDE=2" "PBRS_WIDE=0"      (PBRS_WIDE: bit 1 lets k_shadow walk four-wide nodes, its only bit)
# (PBRS_WIDE without bit 1 switches k_shadow's four-wide walk off: the tests that assert which walk the PRODUCT takes — wide_any, feature bit 4 —
#  fail by design under it; profiles/r04z_dev_parity.log.)
lib=$1; shift
for v in "$@"; do
  echo "== $v"
  env $v PBRS_GPU_LIB=$PWD/pbrs_amd/lib/abl_$lib.so timeout -k 10 400 python -m pytest tests -m gpu -q -rf 2>&1 | grep -E "^FAILED|passed|failed"
done
