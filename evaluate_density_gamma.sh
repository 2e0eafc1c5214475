#!/bin/sh
# evaluate_density_gamma.sh — CLARK's script of the same name: the density of assignments per gamma score of result CSVs
# (exe/evaluate_density --gamma): -F <result.csv> [<result.csv> ...].  The report goes to stdout: per bin of 0.01 from 0.00 to 1.00
# the assigned objects of the bin and the objects --min-gamma <that value> keeps.
DIR=$(dirname "$0")
if [ $# -lt 1 ]; then
  echo "Usage: $0 -F <result.csv> [<result.csv> ...]"
  exit 0
fi
exec "$DIR/exe/evaluate_density" "$@" --gamma
