#!/bin/sh
# split_reads.sh — the reads of a result CSV written out as classified and unclassified files (exe/split_reads), on the CPU:
# -F <result.csv> -O <reads.fa|fq> [--classified-out <file>] [--unclassified-out <file>] [-c <min confidence>] [-g <min gamma>]
# [--highconfidence].  The same files exe/cuCLARK --classified-out / --unclassified-out writes while it classifies.
DIR=$(dirname "$0")
if [ $# -lt 1 ]; then
  echo "Usage: $0 -F <result.csv> -O <reads.fa|fq> [--classified-out <file>] [--unclassified-out <file>] [-c <conf>] [-g <gamma>] [--highconfidence]"
  exit 0
fi
exec "$DIR/exe/split_reads" "$@"
