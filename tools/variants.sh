#!/bin/bash
# Build variants of libucdir_hip.so for same-box A/B runs:  tools/variants.sh name1:"-DFLAG1 -DFLAG2" name2:"" ...
# -> ucdir_amd/variants/libucdir_<name>.so  (git-ignored; each variant is built by ucdir_amd/build.py with the flags added)
R=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p $R/ucdir_amd/variants
cd $R
for spec in "$@"; do
  name=${spec%%:*}; flags=${spec#*:}
  python -c "import sys; from ucdir_amd import build; build.build(force=True, extra_flags=tuple(sys.argv[2].split()), out=sys.argv[1])" \
    $R/ucdir_amd/variants/libucdir_$name.so "$flags" &
done
wait
ls -la $R/ucdir_amd/variants/
