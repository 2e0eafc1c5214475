#!/bin/sh
# estimate_abundance.sh — CLARK's third step: the abundance profile of result CSVs (exe/estimate_abundance), with CLARK's calling
# convention: -F <result.csv> [<result.csv> ...] [-c <min confidence>] [-g <min gamma>] [-a <min abundance>] [--highconfidence],
# and [--rank-report <file> [--lineage <tsv>]] for the rank roll-up report of --extended result CSVs (passed on as they are).
# Unless -D is given, the database directory of ./.settings (set_targets.sh) is passed on: names and lineages then come from the
# taxonomy next to it.  The table goes to stdout.
DIR=$(dirname "$0")
if [ $# -lt 1 ]; then
  echo "Usage: $0 -F <result.csv> [<result.csv> ...] [-D <database directory>] [-c <conf>] [-g <gamma>] [-a <min %>] [--highconfidence] [--rank-report <file> [--lineage <tsv>]]"
  exit 0
fi
for a in "$@"; do
  [ "$a" = "-D" ] && exec "$DIR/exe/estimate_abundance" "$@"
done
if [ -f ./.settings ]; then
  DB=$(sed -n 's/^-D //p' ./.settings | head -n 1)
  [ -n "$DB" ] && exec "$DIR/exe/estimate_abundance" "$@" -D "$DB"
fi
exec "$DIR/exe/estimate_abundance" "$@"
