# Build a diagnostic variant of libqconvnet.so (never the product library):
#   bash tools/build_variant.sh NAME TU "-DFOO=1 ..." [PATCH]
# compiles csrc/TU.hip (conv3x3, classifier, convgemm, ...) with the extra
# hipcc defines — after applying PATCH (a file under tools/patches/, e.g.
# grid_probe.patch) to a copy of the sources in build/var_NAME/src when one is
# given — and links it with the product's other objects (the Makefile's own
# list, built first if need be) into
# convnet-quantization_amd/qconvnet/libqconvnet_NAME.so; load it with QCN_LIB.
set -e
NAME=$1 TU=$2 DEFS=$3 PATCH=$4
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
cd "$ROOT/convnet-quantization_amd/csrc"
[ -f "$TU.hip" ] || { echo "usage: build_variant.sh NAME TU \"DEFINES\" [PATCH]  (no csrc/$TU.hip)" >&2; exit 2; }
make -s -j8
VAR=build/var_$NAME
mkdir -p $VAR
SRC=$TU.hip
if [ -n "$PATCH" ]; then
  rm -rf $VAR/src && mkdir -p $VAR/src
  cp *.hip *.hpp $VAR/src/
  (cd $VAR/src && patch -s -p3 < "$ROOT/$PATCH")
  SRC=$VAR/src/$TU.hip
fi
# the product's compile line and object list, with this one object replaced
make -s variant VAR_TU=$TU VAR_SRC=$SRC VAR_DIR=$VAR VAR_FLAGS="$DEFS" VAR_OUT=../qconvnet/libqconvnet_$NAME.so
