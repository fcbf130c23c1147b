#!/bin/bash
# debug build of the library with phase stamps in the LU leaf kernel (-DGSI_LU_TRACE) -> tools/libgsi_hip_trace.so
set -e
cd "$(dirname "$0")/../geostatinversion.jl_amd"
python build.py > /dev/null
mkdir -p /tmp/tracebuild
OBJS=""
for f in $(python -c 'import build; print(" ".join(s for s in build.SOURCES if s != "panel_lu_leaf.hip"))'); do OBJS="$OBJS build/${f/./_}.o"; done
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -DGSI_LU_TRACE -x hip -c csrc/panel_lu_leaf.hip -o /tmp/tracebuild/panel_lu_leaf_hip.o
/opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -Wl,-Bsymbolic -o ../tools/libgsi_hip_trace.so $OBJS /tmp/tracebuild/panel_lu_leaf_hip.o -ldl
