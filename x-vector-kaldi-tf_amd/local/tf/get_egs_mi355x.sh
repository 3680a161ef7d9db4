#!/usr/bin/env bash
# Training examples for local/tf/train_dnn.py from a RAW data directory on the MI355X -- what run.sh stage 3
# (prepare_feats_for_egs.sh + the length / speaker filters) and local/tf/get_egs.sh do with Kaldi binaries and a second copy of all
# features, without either (make_egs.py, xvector_amd/egs.py).  <data> holds feats.scp (raw MFCCs), vad.scp, utt2spk, spk2utt; data
# dirs with a segments file are refused.  Options as get_egs.sh (--name value), plus --min-len / --min-num-utts of stage 3 and
# --seed for the held-out lists (a seeded Python shuffle, not utils/shuffle_list.pl's stream).
# Usage: get_egs_mi355x.sh [options] <data> <egs-dir>
set -euo pipefail
stage=0
nj=6
min_frames_per_chunk=200
max_frames_per_chunk=400
frames_per_iter=10000000
frames_per_iter_diagnostic=100000
num_diagnostic_archives=1
num_heldout_utts=200
num_repeats=10
minibatch_size=128
min_len=500
min_num_utts=8
seed=0
cmn_window=300
while [[ $# -gt 0 && $1 == --* ]]; do
  name=${1#--}; name=${name//-/_}
  [[ $# -ge 2 && -n ${!name+x} ]] || { echo "$0: unknown option $1" >&2; exit 1; }
  printf -v "$name" '%s' "$2"; shift 2
done
[[ $# -eq 2 ]] || { sed -n 2,8p "$0"; exit 1; }
data=$1; egs_dir=$2
here=$(cd "$(dirname "$0")" && pwd)
for f in feats.scp vad.scp utt2spk spk2utt; do [[ -f $data/$f ]] || { echo "$0: expected file $data/$f" >&2; exit 1; }; done
if [[ -f $data/segments ]]; then
  echo "$0: $data/segments exists: segmented recordings are not supported" >&2
  exit 1
fi
temp=$egs_dir/temp
mkdir -p "$egs_dir/info" "$temp"

if [[ $stage -le 0 ]]; then
  echo "$0: Removing silence on paper, filtering utterances and speakers, preparing train and validation lists"
  python "$here/make_egs.py" prepare --data "$data" --out-dir "$temp/no_sil" --min-len "$min_len" --min-num-utts "$min_num_utts"
  python "$here/make_egs.py" lists --utt2spk "$temp/no_sil/utt2spk" --spk2utt "$temp/no_sil/spk2utt" \
      --utt2num-frames "$temp/no_sil/utt2num_frames" --temp "$temp" --num-heldout-utts "$num_heldout_utts" --seed "$seed"
fi
feat_dim=$(cat "$temp/no_sil/feat_dim")
num_train_archives=$(python "$here/make_egs.py" info --egs-dir "$egs_dir" --feat-dim "$feat_dim" --num-repeats "$num_repeats" \
    --frames-per-iter "$frames_per_iter" --num-diagnostic-archives "$num_diagnostic_archives")
echo "$0: Producing $num_train_archives archives for training"
[[ $nj -le $num_train_archives ]] || nj=$num_train_archives

if [[ $stage -le 1 ]]; then
  common=(--minibatch-size="$minibatch_size" --min-frames-per-chunk="$min_frames_per_chunk"
          --max-frames-per-chunk="$max_frames_per_chunk" --egs-dir="$egs_dir")
  echo "$0: Allocating training examples"
  python "$here/make_egs.py" allocate --num-repeats="$num_repeats" --num-jobs="$nj" --frames-per-iter="$frames_per_iter" \
      --num-archives="$num_train_archives" --utt2len-filename="$temp/utt2num_frames.train" \
      --utt2int-filename="$temp/utt2int.train" "${common[@]}"
  for set in train_subset valid; do
    echo "$0: Allocating $set examples"
    python "$here/make_egs.py" allocate --prefix="$set" --num-repeats=8 --num-jobs=1 --randomize-chunk-length=false \
        --frames-per-iter="$frames_per_iter_diagnostic" --num-archives="$num_diagnostic_archives" \
        --utt2len-filename="$temp/utt2num_frames.$set" --utt2int-filename="$temp/utt2int.$set" "${common[@]}"
  done
fi

if [[ $stage -le 3 ]]; then
  random_seed=2468
  common=(--random-seed="$random_seed" --feature-dim="$feat_dim" --minibatch-size="$minibatch_size" --shuffle=True
          --egs-dir="$egs_dir" --feats-scp "$data/feats.scp" --vad-scp "$data/vad.scp" --cmn-window "$cmn_window")
  echo "$0: Generating training examples on disk"
  for g in $(seq "$nj"); do
    python "$here/make_egs.py" write --outputs-file="$temp/outputs.$g" "${common[@]}"
  done
  for set in train_subset valid; do
    echo "$0: Generating $set examples on disk"
    python "$here/make_egs.py" write --prefix="$set" --outputs-file="$temp/${set}_outputs.1" "${common[@]}"
  done
fi
echo "$0: Finished preparing training examples"
