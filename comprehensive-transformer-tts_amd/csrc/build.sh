#!/bin/bash
# Build libctts_hip.so for gfx950 (MI355X).  hipcc cross-compiles without a GPU.
#   CTTS_VARIANT=name CTTS_CXXFLAGS="-DCTTS_BK=64 -DCTTS_GEMM_WAVES=2" build.sh  -> libctts_hip_name.so (tuning A/B builds)
set -e
cd "$(dirname "$0")"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
SUF=${CTTS_VARIANT:+_$CTTS_VARIANT}
OUT=libctts_hip${SUF}.so
OBJ=.obj${SUF}
mkdir -p $OBJ
SRCS="gemm.hip gemm_sk.hip gemm_ws.hip gemm_pl.hip gemm_plw.hip attn.hip lr.hip norm.hip elementwise.hip conformer.hip align.hip prosody.hip optim.hip loss.hip mel.hip pitch.hip comm.hip vocoder.hip vocoder_h.hip fastformer.hip griffinlim.hip pitchtrack.hip preprocess.hip metrics.hip resample.hip loudness.hip wavmetrics.hip speaker.hip"
# every object depends on every header (and on this script): one list for both staleness tests
DEPS="ctts_common.h fft_common.h gemm_common.h gemm_pl_common.h planes_common.h vocoder_common.h sk_plan.h sk_handoff.h batch_plan.h ../../include/ctts.h build.sh"
newest=$(ls -t $SRCS $DEPS | head -1)
if [ -f "$OUT" ] && [ "$OUT" -nt "$newest" ]; then echo "$OUT up to date"; exit 0; fi
newest_dep=$(ls -t $DEPS | head -1)
objs=""
for s in $SRCS; do
  o="$OBJ/${s%.hip}.o"
  if [ ! -f "$o" ] || [ "$s" -nt "$o" ] || [ "$newest_dep" -nt "$o" ]; then
    $HIPCC --offload-arch=gfx950 -O3 -std=c++17 -fPIC $CTTS_CXXFLAGS -c "$s" -o "$o" &
  fi
  objs="$objs $o"
done
wait
$HIPCC --offload-arch=gfx950 -shared -fPIC $objs -ldl -o $OUT
echo "built $(pwd)/$OUT"
