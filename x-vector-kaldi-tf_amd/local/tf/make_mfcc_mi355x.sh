#!/usr/bin/env bash
# MFCC features of one Kaldi data directory on the MI355X -- what steps/make_mfcc.sh does with nj CPU jobs and Kaldi binaries
# (mfcc_vad.py compute-mfcc-feats): writes <out-dir>/raw_mfcc_<name>.{ark,scp} and puts feats.scp and utt2num_frames into the
# data dir.  vad.scp is left as it is: stage 2 of the recipe copies the clean VAD to the augmented copies.  wav.scp entries
# written by Kaldi's reverberate_data_dir.py / augment_data_dir.py are evaluated on the GPU (no wav-reverberate binary).
# Data dirs with a segments file are refused (not supported).
# --compress true writes the features as Kaldi CompressedMatrix records, encoded on the GPU (a quarter of the bytes).  The default
# here is false; Kaldi's steps/make_mfcc.sh defaults to true.
# Usage: make_mfcc_mi355x.sh [--compress true|false] <data-dir> <mfcc.conf> <out-dir>
set -euo pipefail
compress=false
if [[ ${1:-} == --compress ]]; then
  [[ ${2:-} == true || ${2:-} == false ]] || { echo "$0: --compress takes true or false" >&2; exit 1; }
  compress=$2; shift 2
fi
[[ $# -eq 3 ]] || { sed -n 2,9p "$0"; exit 1; }
data=$1; mfcc_conf=$2; dir=$3
here=$(cd "$(dirname "$0")" && pwd)
for f in "$data/wav.scp" "$mfcc_conf"; do [[ -f $f ]] || { echo "$0: no such file $f" >&2; exit 1; }; done
if [[ -f $data/segments ]]; then
  echo "$0: $data/segments exists: segmented recordings are not supported (extract the segments into a wav.scp first)" >&2
  exit 1
fi
name=$(basename "$data")
mkdir -p "$dir/log"
dir=$(cd "$dir" && pwd)
python "$here/mfcc_vad.py" compute-mfcc-feats --compress=$compress --config="$mfcc_conf" --write-num-frames="ark,t:$data/utt2num_frames" \
    "scp:$data/wav.scp" "ark,scp:$dir/raw_mfcc_$name.ark,$dir/raw_mfcc_$name.scp" 2>&1 | tee "$dir/log/make_mfcc_$name.log"
cp "$dir/raw_mfcc_$name.scp" "$data/feats.scp"
