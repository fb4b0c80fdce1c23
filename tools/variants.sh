#!/bin/bash
# Diagnostic: build variants of the plain kernel object and of the runtime with extra -D flags into audio_codec_amd/_var/ (git-ignored).
# The flags go to both files (-DLC3_DUP acts on the runtime, -DFM_CAP on a kernel, -DFRONT_FPW on both); every other object is the product's (build it first).
# usage: tools/variants.sh name1 "-DFOO=1" name2 "-DBAR=2" ...      then on the GPU box: tools/variants_run.sh
set -e
cd "$(dirname "$0")/../audio_codec_amd/csrc"
mkdir -p ../_var
FLAGS="-Os -ffp-contract=off --offload-arch=gfx950 -fPIC -Wno-unused-value"
REST=$(make -s print-objs | tr ' ' '\n' | grep -v -e '/lc3_kernels\.o$' -e '/lc3_runtime\.o$')
while [ $# -ge 2 ]; do
  n=$1; d=$2; shift 2
  ( hipcc $FLAGS $d -c lc3_kernels.hip -o ../_var/k_$n.o 2>../_var/build_$n.log && hipcc $FLAGS $d -c lc3_runtime.hip -o ../_var/r_$n.o 2>>../_var/build_$n.log && hipcc --offload-arch=gfx950 -shared -fPIC -o ../_var/lib_$n.so ../_var/k_$n.o ../_var/r_$n.o $REST -lm && rm ../_var/k_$n.o ../_var/r_$n.o && echo built $n ) &
  while [ $(jobs -r | wc -l) -ge 4 ]; do sleep 1; done
done
wait
