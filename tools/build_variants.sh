#!/bin/bash
# Build variants of the env library THE PRODUCT'S WAY (vectoriser + isa_fix pass, stackrl_amd/build.py) into ab_libs/ for a
# same-box A / B with tools/ab_bench.sh:  tools/build_variants.sh name1 "flags1" name2 "flags2" ...
cd "$(dirname "$0")/.." || exit 1
mkdir -p ab_libs && rm -f ab_libs/lib*.so ab_libs/variants.txt
while [ $# -ge 2 ]; do
  name=$1; flags=$2; shift 2
  variant=$(SRL_EXTRA_FLAGS="$flags" python -c "
from stackrl_amd import build as b
b.build_library('env', 'ab_libs/lib_$name.so')
print(b.info('ab_libs/lib_$name.so')['variant'])") || exit 1
  echo "lib_$name.so: ${flags:-(product build)} [$variant]" >> ab_libs/variants.txt
done
cat ab_libs/variants.txt
