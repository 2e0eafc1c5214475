// cli_main.cpp — command line of exe/cuCLARK and exe/cuCLARK-l (one binary; the light variant is selected by the
// program name or --light).  Flag surface, defaults, messages and exit codes follow the reference's main.cc:74-320,
// so classify_metagenome.sh can exec this binary unchanged (classify_metagenome.sh:155-159).
// Additions that do not change defaults: --light, --htsize <n> (table size = size of the .sz file; the reference
// fixes it at compile time, parameters.hh:39 / parameters_light_hh:40).
#include <stdio.h>
#include <stdlib.h>
#include <unistd.h>
#include <string.h>

#include <sys/stat.h>
#include <sys/time.h>

#include <fstream>
#include <iostream>
#include <iterator>
#include <string>

#include "abundance_table.hpp"
#include "classifier.hpp"
#include "density_report.hpp"
#include "kmer_report.hpp"
#include "kraken_report.hpp"
#include "mic_abund.h"

#define MAXK 32
#define SFACTORMAX 30
#define VERSION "1.1"
static const uint64_t HTSIZE_FULL = 1610612741ull, HTSIZE_LIGHT = 57777779ull;

static bool valid_file(const char* f) {
  FILE* fd = fopen(f, "r");
  if (!fd) return false;
  fclose(fd);
  return true;
}

static void print_usage(const char* prog) {
  std::cout << "\n" << prog << " -- MI355X-native k-mer read classifier with CuCLARK's command line\n\n";
  std::cout << prog << " -k <kmerSize> -t <minFreqTarget> -T <fileTargets> -D <directoryDB/> -O <fileObjects> -R <fileResults> "
               "-n <numberofthreads> -b <numberofbatches> -d <numberofdevices> ...\n\n";
  std::cout << "Definitions of parameters (cf. README of CuCLARK):\n";
  std::cout << "-k <kmerSize>,       k-mer length, integer in [2,32] (default 31; the light variant always uses 27)\n";
  std::cout << "-t <minFreqTarget>,  minimum k-mer frequency in targets (part of the database name)\n";
  std::cout << "-T <fileTargets>,    targets definition: one line per reference file, '<file> <label>'\n";
  std::cout << "-D <directoryDB/>,   directory of the database files db_central_k*_t*_s*_m*.tsk.{sz,ky,lb}\n";
  std::cout << "-O <fileObjects>,    FASTA/FASTQ file of objects (or a list of files when -R names an existing list)\n";
  std::cout << "-P <file1> <file2>,  paired-end FASTQ files\n";
  std::cout << "-R <fileResults>,    results file name ('.csv' is appended)\n";
  std::cout << "-n <numberofthreads> host threads (raises the number of batches if needed)\n";
  std::cout << "-b <numberofbatches> batches the objects are split into (>= threads)\n";
  std::cout << "-d <numberofdevices> GPUs to use (default: all)\n";
  std::cout << "-g <iteration>,      gap for the light database name (>= 4)\n";
  std::cout << "-s <factor>,         sampling factor in [2," << SFACTORMAX << "]\n";
  std::cout << "--db-sharded,        several GPUs: the table is cut into parts held by different GPUs (the mode of CuCLARK's -d); default: the table\n"
               "                     is replicated on every GPU and the batches are dealt to the GPUs\n";
  std::cout << "--parts <P>,         with --db-sharded: number of parts (divides -d; the GPUs form d/P groups that share the reads);\n"
               "                     default: the smallest number of parts that fit a GPU's memory\n";
  std::cout << "--abundance <file>,  also count the abundance profile of the objects (CLARK's estimate_abundance table) into <file>;\n"
               "                     without -R no result CSV is written (summary-only run)\n";
  std::cout << "--rank-report <file> [--lineage <tsv>],  also resolve every object at the lowest rank whose confidence passes --min-confidence\n"
               "                     and count the objects per rank and group into <file>; the lineage of the targets comes from <tsv>\n"
               "                     (label<TAB>name_1<TAB>...<TAB>name_L per target) or from <DB>/../taxonomy; works without -R like --abundance\n";
  std::cout << "--density <file>,    also count the objects per confidence score and per gamma score (bins of 0.01, and the joint table) into <file>:\n"
               "                     CLARK's evaluate_density reports, whose cumulative columns are what --min-confidence / --min-gamma keep;\n"
               "                     works without -R like --abundance\n";
  std::cout << "--kmer-report <file>, also sketch the distinct k-mers the objects hit in every target (HyperLogLog, 16384 registers per target) into\n"
               "                     <file>: Name,Reads,Kmers,DistinctKmers,Duplication - many reads over few distinct k-mers (a high duplication) mark\n"
               "                     a low-complexity or contamination artefact; Reads as in --abundance; not with --db-sharded or a list of files;\n"
               "                     works without -R like --abundance\n";
  std::cout << "--hit-maps <file>,   also write, per object, the runs of k-mer assignments along it into <file>: Object_ID,Hit_map with tokens\n"
               "                     <target>:<k-mers> (0: no target) joined by blanks, | between two stretches of nucleotides (an N, a masked base, the\n"
               "                     two mates of -P) - where the hits fall: a chimera reads A:90 0:30 B:70; -O and -P; not with --db-sharded or a\n"
               "                     list of files; works without -R like --abundance\n";
  std::cout << "--kraken-out <file>,  also write Kraken's per-read file into <file>, one line per object and no header line:\n"
               "                     C|U<TAB>name<TAB>label of the 1st assignment (0 on a U line)<TAB>Length<TAB>the hit map as <target>:<k-mers> tokens, |:|\n"
               "                     between two stretches of nucleotides, 0:0 for an object without k-mers.  C as --classified-out decides it under\n"
               "                     --min-confidence / --min-gamma; the third column is the target's label, not an LCA; one Length, not a|b, for -P.\n"
               "                     -O and -P; not with --hit-maps, --db-sharded or a list of files; works without -R like --abundance\n";
  std::cout << "--kraken-report <file> [--lineage <tsv>] [--kraken-target-rank <rank>],  also write Kraken's sample report of the abundance\n"
               "                     counts into <file>: %, clade reads, taxon reads, rank code, taxid, indented name.  The tree is the lineage of\n"
               "                     --rank-report (from <tsv>, else <DB>/../taxonomy; with neither the targets hang under the root); the targets\n"
               "                     get the code of <rank> (default species); works without -R like --abundance\n";
  std::cout << "--kmer-coverage <file>, the k-mer report with two more columns: Name,Reads,Kmers,DistinctKmers,Duplication,TargetKmers,Coverage -\n"
               "                     TargetKmers, the target's k-mers in the resident table, from a census of the table on the device when it is\n"
               "                     loaded (every k-mer of the database is probed through the table; one that does not come back under its label\n"
               "                     fails the load), and Coverage = min(DistinctKmers, TargetKmers) / TargetKmers: the fraction of the target the\n"
               "                     objects touched; with -s the coverage is relative to the sampled (resident) k-mers; alone or next to\n"
               "                     --kmer-report and -R; not with --db-sharded or a list of files\n";
  std::cout << "--classified-out <file>,  also write the objects that are assigned under --min-confidence / --min-gamma into <file>, as they are in -O\n";
  std::cout << "--unclassified-out <file>,  also write the other objects (no hit, or dropped by the filter) into <file>; either option alone or both;\n"
               "                     one -O input only (not -P, not a list of files); the names are taken as given; work without -R like --abundance\n";
  std::cout << "--min-confidence <c>, --min-gamma <g>, --highconfidence (= --min-confidence 0.75 --min-gamma 0.03), --min-abundance <a>:\n"
               "                     the filters of the abundance profile (CLARK's -c, -g, --highconfidence, -a; defaults 0.5, 0, 0)\n";
  std::cout << "--min-base-quality <Q> [--quality-offset 33|64],  FASTQ: bases of Phred quality below Q (integer in [1,93]; quality characters\n"
               "                     at offset 33, or 64) are treated as N: they belong to no k-mer.  Length, names and gamma's denominator\n"
               "                     do not change; FASTA input has no qualities and is unaffected\n";
  std::cout << "--mask-low-complexity <level>,  bases whose surrounding 32-nucleotide window has a DUST score above level/10 (integer in\n"
               "                     [1,149]; 20 is DUST's customary level) are treated as N: homopolymers and microsatellites belong to\n"
               "                     no k-mer.  FASTA and FASTQ; Length, names and gamma's denominator do not change\n";
  std::cout << "--tsk, --extended, --light, --htsize <n>, --help, --version\n\n";
}

int main(int argc, char** argv) {
  const char* slash = strrchr(argv[0], '/');
  const std::string prog = slash ? slash + 1 : argv[0];
  if (argc == 2) {
    std::string val(argv[1]);
    if (val == "--help" || val == "--HELP") { print_usage(argv[0]); return 0; }
    if (val == "--version" || val == "--VERSION") {
      std::cout << "Version: " << VERSION << " (mi-clark MI355X engine; CuCLARK Copyright 2016-2017 Robin Kobus, rkobus@students.uni-mainz.de)" << std::endl;
      std::cout << "Based on CLARK version 1.1.3 (UCR CS&E. Copyright 2013-2016 Rachid Ounit, rouni001@cs.ucr.edu) " << std::endl;
      return 0;
    }
  }
  // cuCLARK --merge-pairs <file1> <file2> <out.fa> [serial|parallel [threads [batch_bytes [threshold_byte]]]]: the paired-end merge
  // alone (file.cc:205-268: the reference writes <file1>_ConcatenatedByCLARK.fa and classifies that), no device involved.
  // "parallel" prints "gave up" and exits 3 when the loaders' merger hands the files to the serial reader.  threshold_byte: the
  // merge as --min-base-quality runs it on the host (offset + Q, mic_qmask.h).
  if (argc >= 5 && std::string(argv[1]) == "--merge-pairs") {
    try {
      std::string text;
      const bool par = argc > 5 && std::string(argv[5]) == "parallel";
      const uint32_t qm = argc > 8 ? (uint32_t)atoi(argv[8]) & 255u : 0u;
      if (par) {
        const unsigned th = argc > 6 ? (unsigned)atoi(argv[6]) : 4u;
        const size_t bb = argc > 7 ? (size_t)strtoull(argv[7], nullptr, 10) : (size_t)1 << 20;
        if (!mic::merge_paired_parallel(argv[2], argv[3], th ? th : 1u, bb ? bb : 1, text, qm)) { std::cerr << "gave up" << std::endl; return 3; }
      } else text = mic::merge_paired(argv[2], argv[3], qm);
      FILE* f = fopen(argv[4], "wb");
      if (!f || fwrite(text.data(), 1, text.size(), f) != text.size() || fclose(f) != 0) { std::cerr << "Failed to write " << argv[4] << std::endl; return 1; }
      return 0;
    } catch (const std::exception& ex) {
      std::cerr << ex.what() << std::endl;
      return 1;
    }
  }
  // cuCLARK --strip-fastq <in.fq> <out> [piece_bytes [scalar|bench]]: the loaders' FASTQ stripper alone (header + sequence line
  // of every record), fed in pieces; "bench" prints both forms' rates instead of writing
  if (argc >= 4 && std::string(argv[1]) == "--strip-fastq") {
    try {
      const size_t piece = argc > 4 ? (size_t)strtoull(argv[4], nullptr, 10) : (size_t)1 << 20;
      const std::string mode = argc > 5 ? argv[5] : "";
      std::string in;
      if (mode != "loaders") {
        std::ifstream f(argv[2], std::ios::binary);
        in.assign((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
      }
      if (mode == "loaders") {
        const unsigned th = argc > 6 ? (unsigned)atoi(argv[6]) : 8u;
        const bool mm = argc > 7 && std::string(argv[7]) == "mmap";
        for (int rep = 0; rep < 3; ++rep)
          std::cout << (mm ? "mmap" : "pread") << " chunk " << piece << " threads " << th << ": " << mic::strip_fastq_loaders_rate(argv[2], piece, th ? th : 1, mm) << " GB/s" << std::endl;
        return 0;
      }
      if (mode == "bench") {
        for (int sc = 1; sc >= 0; --sc) {
          struct timeval a, b; gettimeofday(&a, nullptr);
          size_t tot = 0;
          tot = 5 * mic::strip_fastq_text(in, piece ? piece : 1, sc != 0, 5).size();
          gettimeofday(&b, nullptr);
          const double sec = (b.tv_sec - a.tv_sec) + (b.tv_usec - a.tv_usec) * 1e-6;
          std::cout << (sc ? "scalar" : "vector") << ": " << 5.0 * in.size() / sec / 1e9 << " GB/s in (" << tot / 5 << " bytes out)" << std::endl;
        }
        return 0;
      }
      const std::string out = mic::strip_fastq_text(in, piece ? piece : 1, mode == "scalar");
      FILE* o = fopen(argv[3], "wb");
      if (!o || fwrite(out.data(), 1, out.size(), o) != out.size() || fclose(o) != 0) { std::cerr << "Failed to write " << argv[3] << std::endl; return 1; }
      return 0;
    } catch (const std::exception& ex) {
      std::cerr << ex.what() << std::endl;
      return 1;
    }
  }
  if (argc < 6) {
    std::cerr << "To run " << argv[0] << ", at least four  parameters are necessary:\n";
    std::cerr << "filename of the targets definition, directory of database, filename for objects, filename for results." << std::endl;
    print_usage(argv[0]);
    return -1;
  }
  mic::Options o;
  size_t k = 31, cpu = 1, batches = 1, devices = 0, gap = 0;
  uint32_t minT = 0, sfactor = 1;
  bool ext = false, tsk = false;
  bool light = prog.size() >= 2 && prog.compare(prog.size() - 2, 2, "-l") == 0;
  uint64_t htsize_override = 0;
  bool db_sharded = false;
  size_t parts = 0;
  int i_targets = -1, i_objects = -1, i_objects2 = -1, i_folder = -1, i_results = -1;
  std::string abundance, rank_report, lineage, density, kmer_report, kmer_coverage, classified_out, unclassified_out, hit_maps, kraken_out, kraken_report, kraken_rank = "species";
  mic_abund_filter ab_filter = {5, 10, 0, 1};
  uint64_t ab_min_num = 0, ab_min_den = 1;
  long min_q = 0, q_offset = 0;          // --min-base-quality, --quality-offset (0: not given)
  long lowc = 0;                         // --mask-low-complexity (0: not given)
  // a whole decimal integer, nothing before or behind it
  auto parse_int = [](const char* s, long& v) {
    if (!*s || strlen(s) > 9) return false;
    for (const char* c = s; *c; ++c) if (*c < '0' || *c > '9') return false;
    v = atol(s);
    return true;
  };

  for (int i = 1; i < argc; i++) {
    std::string val(argv[i]);
    auto need = [&](const char* msg) { if (++i >= argc) { std::cerr << msg << std::endl; exit(1); } };
    if (val == "-k") {
      need("Please specify the k-mer length!");
      k = (size_t)atoi(argv[i]);
      if (k <= 1 || k > MAXK) { std::cerr << "The k-mer length should be in [2," << MAXK << "]." << std::endl; exit(1); }
      continue;
    }
    if (val == "-t") {
      need("Please specify the minimum frequency (targets)!");
      minT = (uint32_t)atoi(argv[i]);
      if (minT >= 65536) { std::cerr << "The min k-mer frequency should be in [0,65535]." << std::endl; exit(1); }
      continue;
    }
    if (val == "-n") {
      need("Please specify the number of threads!");
      int c = atoi(argv[i]);
      if (c < 1) { std::cerr << "The number of threads should be higher than 0." << std::endl; exit(1); }
      cpu = (size_t)c;
      if (batches < cpu) batches = cpu;
      continue;
    }
    if (val == "--tsk") { tsk = true; continue; }
    if (val == "--extended") { ext = true; continue; }
    if (val == "--db-sharded") { db_sharded = true; continue; }
    if (val == "--parts") {
      need("Please specify the number of parts of the table!");
      int p = atoi(argv[i]);
      if (p < 1 || p > 64) { std::cerr << "The number of parts should be in [1,64]." << std::endl; exit(1); }
      parts = (size_t)p; db_sharded = true;
      continue;
    }
    if (val == "--light") { light = true; continue; }
    if (val == "--abundance") { need("Please specify the file of the abundance profile!"); abundance = argv[i]; continue; }
    if (val == "--classified-out") { need("Please specify the file of the classified objects!"); classified_out = argv[i]; if (classified_out.empty()) { std::cerr << "Please specify the file of the classified objects!" << std::endl; exit(1); } continue; }
    if (val == "--unclassified-out") { need("Please specify the file of the unclassified objects!"); unclassified_out = argv[i]; if (unclassified_out.empty()) { std::cerr << "Please specify the file of the unclassified objects!" << std::endl; exit(1); } continue; }
    if (val == "--density") { need("Please specify the file of the density report!"); density = argv[i]; continue; }
    if (val == "--kmer-coverage") { need("Please specify the file of the k-mer coverage report!"); kmer_coverage = argv[i]; if (kmer_coverage.empty()) { std::cerr << "Please specify the file of the k-mer coverage report!" << std::endl; exit(1); } continue; }
    if (val == "--kmer-report") { need("Please specify the file of the k-mer report!"); kmer_report = argv[i]; if (kmer_report.empty()) { std::cerr << "Please specify the file of the k-mer report!" << std::endl; exit(1); } continue; }
    if (val == "--hit-maps") { need("Please specify the file of the hit maps!"); hit_maps = argv[i]; if (hit_maps.empty()) { std::cerr << "Please specify the file of the hit maps!" << std::endl; exit(1); } continue; }
    if (val == "--kraken-out") { need("Please specify the file of the Kraken output!"); kraken_out = argv[i]; if (kraken_out.empty()) { std::cerr << "Please specify the file of the Kraken output!" << std::endl; exit(1); } continue; }
    if (val == "--kraken-report") { need("Please specify the file of the Kraken report!"); kraken_report = argv[i]; if (kraken_report.empty()) { std::cerr << "Please specify the file of the Kraken report!" << std::endl; exit(1); } continue; }
    if (val == "--kraken-target-rank") { need("Please specify the rank of the targets!"); kraken_rank = argv[i]; continue; }
    if (val == "--rank-report") { need("Please specify the file of the rank report!"); rank_report = argv[i]; continue; }
    if (val == "--lineage") {
      need("Please specify the lineage file!");
      lineage = argv[i];
      if (!valid_file(argv[i])) { std::cerr << "Failed to find/read the lineage file: " << argv[i] << std::endl; exit(1); }
      continue;
    }
    if (val == "--min-confidence" || val == "--min-gamma" || val == "--min-abundance") {
      need("Please specify the threshold!");
      const bool a = val == "--min-abundance";
      uint64_t* num = a ? &ab_min_num : val == "--min-confidence" ? &ab_filter.conf_num : &ab_filter.gamma_num;
      uint64_t* den = a ? &ab_min_den : val == "--min-confidence" ? &ab_filter.conf_den : &ab_filter.gamma_den;
      if (!mic_abund_parse_text(argv[i], a ? 100 : 1, num, den)) {
        std::cerr << "The value of " << val << " should be a decimal number in [0," << (a ? 100 : 1) << "] with at most 9 decimals: " << argv[i] << std::endl;
        exit(1);
      }
      continue;
    }
    if (val == "--min-base-quality") {
      need("Please specify the minimum base quality!");
      if (!parse_int(argv[i], min_q) || min_q < 1 || min_q > 93) { std::cerr << "The minimum base quality should be an integer in [1,93]: " << argv[i] << std::endl; exit(1); }
      continue;
    }
    if (val == "--mask-low-complexity") {
      need("Please specify the low-complexity level!");
      if (!parse_int(argv[i], lowc) || lowc < 1 || lowc > 149) { std::cerr << "The low-complexity level should be an integer in [1,149]: " << argv[i] << std::endl; exit(1); }
      continue;
    }
    if (val == "--quality-offset") {
      need("Please specify the quality offset!");
      if (!parse_int(argv[i], q_offset) || (q_offset != 33 && q_offset != 64)) { std::cerr << "The quality offset should be 33 or 64: " << argv[i] << std::endl; exit(1); }
      continue;
    }
    if (val == "--highconfidence") { ab_filter.conf_num = 75; ab_filter.conf_den = 100; ab_filter.gamma_num = 3; ab_filter.gamma_den = 100; continue; }
    if (val == "--htsize") {
      need("Please specify the table size!");
      htsize_override = strtoull(argv[i], nullptr, 10);
      if (htsize_override < 2) { std::cerr << "The table size should be >= 2." << std::endl; exit(1); }
      continue;
    }
    if (val == "-T") {
      need("Please specify the targets!");
      i_targets = i;
      if (!valid_file(argv[i])) { std::cerr << "Failed to find/read the file of the targets definition: " << argv[i] << std::endl; exit(1); }
      continue;
    }
    if (val == "-O") {
      need("Please specify the objects!");
      i_objects = i;
      if (!valid_file(argv[i])) { std::cerr << "Failed to find/read the filename of objects: " << argv[i] << std::endl; exit(1); }
      continue;
    }
    if (val == "-P") {
      if (i + 2 >= argc) { std::cerr << "Please specify the paired-end reads!" << std::endl; exit(1); }
      i++;
      i_objects = i; i_objects2 = i + 1;
      if (!valid_file(argv[i++])) { std::cerr << "Failed to find/read " << argv[i - 1] << std::endl; exit(1); }
      if (!valid_file(argv[i])) { std::cerr << "Failed to find/read " << argv[i] << std::endl; exit(1); }
      continue;
    }
    if (val == "-D") {
      need("Please specify the database directory!");
      i_folder = i;
      if (!valid_file(argv[i])) { std::cerr << "Failed to find/read the directory:  " << argv[i] << std::endl; exit(1); }
      continue;
    }
    if (val == "-R") { need("Please specify where to store results!"); i_results = i; continue; }
    if (val == "-g") {
      need("Please specify a gap value!");
      gap = (size_t)atoi(argv[i]);
      if (gap < 4) { std::cerr << "The gap value should be >= 4." << std::endl; exit(1); }
      continue;
    }
    if (val == "-s") {
      need("Please specify a sampling factor value!");
      int s = atoi(argv[i]);
      if (s < 2 || s > SFACTORMAX) { std::cerr << "The sampling factor value should be in the interval [2," << SFACTORMAX << "]." << std::endl; exit(1); }
      sfactor = (uint32_t)s;
      continue;
    }
    if (val == "-b") {
      need("Please specify the number of batches!");
      int b = atoi(argv[i]);
      if (b < 1 || (size_t)b < cpu) { std::cerr << "The number of batches should be higher than the number of threads." << std::endl; exit(1); }
      batches = (size_t)b;
      continue;
    }
    if (val == "-d") {
      need("Please specify the number of devices to use!");
      int d = atoi(argv[i]);
      if (d < 1) { std::cerr << "The number of devices should be higher than 0." << std::endl; exit(1); }
      devices = (size_t)d;
      continue;
    }
    std::cerr << "Failed to recognize option: " << val << std::endl;
    exit(1);
  }
  if (light) {  // CuCLARK-l (main.cc:241-249): k is forced to 27, gap defaults to 4, no sampling
    if (gap == 0) gap = 4;
    k = 27;
    sfactor = 1;
  } else {
    gap = 0;
  }
  if (q_offset && !min_q) { std::cerr << "--quality-offset goes with --min-base-quality <Q>." << std::endl; exit(1); }
  if (!lineage.empty() && rank_report.empty() && kraken_report.empty()) { std::cerr << "--lineage goes with --rank-report <file>." << std::endl; exit(1); }
  const bool split = !classified_out.empty() || !unclassified_out.empty();
  // two names for one file: the same text, or the same inode when both exist
  auto same_file = [](const std::string& a, const std::string& b) {
    if (a.empty() || b.empty()) return false;
    if (a == b) return true;
    struct stat sa, sb;
    return stat(a.c_str(), &sa) == 0 && stat(b.c_str(), &sb) == 0 && sa.st_dev == sb.st_dev && sa.st_ino == sb.st_ino;
  };
  if (!kmer_report.empty()) {      // refused before any device is touched
    if (db_sharded) { std::cerr << "--kmer-report does not take --db-sharded: the sketches are counted behind one GPU's whole table." << std::endl; exit(1); }
    for (int io : {i_objects, i_objects2})
      if (io >= 0 && same_file(kmer_report, argv[io])) { std::cerr << "--kmer-report would overwrite the input: " << kmer_report << std::endl; exit(1); }
    if (i_results >= 0 && same_file(kmer_report, std::string(argv[i_results]) + ".csv")) { std::cerr << "--kmer-report would overwrite the result CSV: " << kmer_report << std::endl; exit(1); }
    if (i_objects >= 0 && i_results >= 0 && mic::Classifier::list_mode(argv[i_objects], argv[i_results])) {
      std::cerr << "--kmer-report does not take list-of-files mode: classify the files one at a time." << std::endl;
      exit(1);
    }
  }
  if (!kmer_coverage.empty()) {      // refused before any device is touched
    if (db_sharded) { std::cerr << "--kmer-coverage does not take --db-sharded: the sketches and the census are counted behind one GPU's whole table." << std::endl; exit(1); }
    for (int io : {i_objects, i_objects2})
      if (io >= 0 && same_file(kmer_coverage, argv[io])) { std::cerr << "--kmer-coverage would overwrite the input: " << kmer_coverage << std::endl; exit(1); }
    if (i_results >= 0 && same_file(kmer_coverage, std::string(argv[i_results]) + ".csv")) { std::cerr << "--kmer-coverage would overwrite the result CSV: " << kmer_coverage << std::endl; exit(1); }
    if (same_file(kmer_coverage, kmer_report)) { std::cerr << "--kmer-coverage names the file of another output: " << kmer_coverage << std::endl; exit(1); }
    if (i_objects >= 0 && i_results >= 0 && mic::Classifier::list_mode(argv[i_objects], argv[i_results])) {
      std::cerr << "--kmer-coverage does not take list-of-files mode: classify the files one at a time." << std::endl;
      exit(1);
    }
  }
  if (!hit_maps.empty()) {      // refused before any device is touched
    if (db_sharded) { std::cerr << "--hit-maps does not take --db-sharded: a map is the labels of one GPU's whole table along the object." << std::endl; exit(1); }
    for (int io : {i_objects, i_objects2})
      if (io >= 0 && same_file(hit_maps, argv[io])) { std::cerr << "--hit-maps would overwrite the input: " << hit_maps << std::endl; exit(1); }
    if (i_results >= 0 && same_file(hit_maps, std::string(argv[i_results]) + ".csv")) { std::cerr << "--hit-maps would overwrite the result CSV: " << hit_maps << std::endl; exit(1); }
    for (const std::string* f : {&abundance, &rank_report, &density, &kmer_report, &kmer_coverage, &classified_out, &unclassified_out})
      if (same_file(hit_maps, *f)) { std::cerr << "--hit-maps names the file of another output: " << hit_maps << std::endl; exit(1); }
    if (i_objects >= 0 && i_results >= 0 && mic::Classifier::list_mode(argv[i_objects], argv[i_results])) {
      std::cerr << "--hit-maps does not take list-of-files mode: classify the files one at a time." << std::endl;
      exit(1);
    }
  }
  if (!kraken_out.empty()) {      // refused before any device is touched
    if (!hit_maps.empty()) { std::cerr << "--kraken-out does not take --hit-maps: the two texts are made in the same buffers, a run writes one of them." << std::endl; exit(1); }
    if (db_sharded) { std::cerr << "--kraken-out does not take --db-sharded: a map is the labels of one GPU's whole table along the object." << std::endl; exit(1); }
    for (int io : {i_objects, i_objects2})
      if (io >= 0 && same_file(kraken_out, argv[io])) { std::cerr << "--kraken-out would overwrite the input: " << kraken_out << std::endl; exit(1); }
    if (i_results >= 0 && same_file(kraken_out, std::string(argv[i_results]) + ".csv")) { std::cerr << "--kraken-out would overwrite the result CSV: " << kraken_out << std::endl; exit(1); }
    for (const std::string* f : {&abundance, &rank_report, &density, &kmer_report, &kmer_coverage, &classified_out, &unclassified_out, &kraken_report})
      if (same_file(kraken_out, *f)) { std::cerr << "--kraken-out names the file of another output: " << kraken_out << std::endl; exit(1); }
    if (i_objects >= 0 && i_results >= 0 && mic::Classifier::list_mode(argv[i_objects], argv[i_results])) {
      std::cerr << "--kraken-out does not take list-of-files mode: classify the files one at a time." << std::endl;
      exit(1);
    }
  }
  if (!kraken_report.empty()) {   // likewise
    for (int io : {i_objects, i_objects2})
      if (io >= 0 && same_file(kraken_report, argv[io])) { std::cerr << "--kraken-report would overwrite the input: " << kraken_report << std::endl; exit(1); }
    if (i_results >= 0 && same_file(kraken_report, std::string(argv[i_results]) + ".csv")) { std::cerr << "--kraken-report would overwrite the result CSV: " << kraken_report << std::endl; exit(1); }
    for (const std::string* f : {&abundance, &rank_report, &density, &kmer_report, &kmer_coverage, &classified_out, &unclassified_out, &hit_maps})
      if (same_file(kraken_report, *f)) { std::cerr << "--kraken-report names the file of another output: " << kraken_report << std::endl; exit(1); }
  }
  if (split) {      // refused before any device is touched
    if (i_objects2 > 0) { std::cerr << "--classified-out / --unclassified-out do not take paired-end input (-P): one -O file only." << std::endl; exit(1); }
    if (same_file(classified_out, unclassified_out)) { std::cerr << "--classified-out and --unclassified-out name the same file: " << classified_out << std::endl; exit(1); }
    for (const std::string* f : {&classified_out, &unclassified_out}) {
      if (i_objects >= 0 && same_file(*f, argv[i_objects])) { std::cerr << "--classified-out / --unclassified-out would overwrite the input: " << *f << std::endl; exit(1); }
      if (i_results >= 0 && same_file(*f, std::string(argv[i_results]) + ".csv")) { std::cerr << "--classified-out / --unclassified-out would overwrite the result CSV: " << *f << std::endl; exit(1); }
    }
    if (i_objects >= 0 && i_results >= 0 && mic::Classifier::list_mode(argv[i_objects], argv[i_results])) {
      std::cerr << "--classified-out / --unclassified-out do not take list-of-files mode: classify the files one at a time." << std::endl;
      exit(1);
    }
  }
  if ((!abundance.empty() || !rank_report.empty() || !density.empty() || !kmer_report.empty() || !kmer_coverage.empty() || !hit_maps.empty() || !kraken_out.empty() || !kraken_report.empty() || split) && i_results < 0 && ext) {
    std::cerr << "--extended writes the result CSV: it needs -R <fileResults>." << std::endl;
    exit(1);
  }
  if (i_targets < 0 || i_folder < 0 || i_objects < 0 || (i_results < 0 && abundance.empty() && rank_report.empty() && density.empty() && kmer_report.empty() && kmer_coverage.empty() && hit_maps.empty() && kraken_out.empty() && kraken_report.empty() && !split)) {
    std::cerr << "Failed to run " << argv[0] << ": at least four  parameters are necessary";
    std::cerr << ": file of targets, directory of database, file of objects, file for results." << std::endl;
    print_usage(argv[0]);
    exit(1);
  }
  o.k = k; o.min_count_t = minT; o.threads = cpu; o.batches = batches; o.devices = devices; o.sampling = sfactor; o.gap = gap;
  o.tsk = tsk; o.extended = ext; o.light = light; o.db_sharded = db_sharded; o.parts = parts;
  if (tsk) std::cerr << "Note: --tsk is accepted for compatibility; the per-target .ht text files (k-mer, count) are not written." << std::endl;
  o.htsize = htsize_override ? htsize_override : (light ? HTSIZE_LIGHT : HTSIZE_FULL);
  o.targets = argv[i_targets];
  o.folder = argv[i_folder];
  if (o.folder.empty() || o.folder.back() != '/') o.folder.push_back('/');
  o.objects = argv[i_objects];
  if (i_objects2 > 0) o.objects2 = argv[i_objects2];
  o.results = i_results >= 0 ? argv[i_results] : "";
  o.abundance = abundance;
  o.abund_filter = ab_filter;
  o.rank_report = rank_report; o.lineage = lineage;
  o.density = density;
  o.kmer_report = kmer_report;
  o.kmer_coverage = kmer_coverage;
  o.hit_maps = hit_maps;
  o.kraken_out = kraken_out; o.kraken_report = kraken_report;
  o.classified_out = classified_out; o.unclassified_out = unclassified_out;
  o.min_quality_byte = min_q ? (uint32_t)((q_offset ? q_offset : 33) + min_q) : 0u;
  o.low_complexity = (uint32_t)lowc;
  mic::Classifier* classifier = nullptr;
  try {
    classifier = new mic::Classifier(o);
    if (i_objects2 > 0) classifier->run_paired(o.objects, o.objects2, o.results);
    else classifier->run(o.objects, o.results);
    if (!abundance.empty()) {   // the profile, named from the taxonomy set_targets.sh leaves next to the database directory
      mic::abund::Taxonomy tax;
      mic::abund::load_taxonomy(o.folder + "../taxonomy", tax);
      const std::string table = mic::abund::format_table(classifier->abundance_counts(), classifier->target_names(), &tax, ab_min_num, ab_min_den);
      FILE* f = fopen(abundance.c_str(), "wb");
      if (!f || fwrite(table.data(), 1, table.size(), f) != table.size() || fclose(f) != 0)
        throw std::runtime_error("Failed to write the abundance profile: " + abundance);
      std::cout << " - Abundance profile stored in " << abundance << std::endl;
    }
    if (!rank_report.empty()) {
      const std::string report = mic::rank::format_report(classifier->rollup_counts(), classifier->lineage());
      FILE* f = fopen(rank_report.c_str(), "wb");
      if (!f || fwrite(report.data(), 1, report.size(), f) != report.size() || fclose(f) != 0)
        throw std::runtime_error("Failed to write the rank report: " + rank_report);
      std::cout << " - Rank report stored in " << rank_report << std::endl;
    }
    if (!classified_out.empty()) std::cout << " - Classified objects stored in " << classified_out << std::endl;
    if (!unclassified_out.empty()) std::cout << " - Unclassified objects stored in " << unclassified_out << std::endl;
    if (!hit_maps.empty()) std::cout << " - Hit maps stored in " << hit_maps << std::endl;
    if (!kraken_out.empty()) std::cout << " - Kraken output stored in " << kraken_out << std::endl;
    if (!kraken_report.empty()) {   // host formatting over the abundance counters, along --rank-report's lineage when there is one
      mic::rank::Lineage kl;
      std::string err;
      if (!mic::kraken::report_lineage(lineage, o.folder + "../taxonomy", classifier->target_names(), kl, err)) throw std::runtime_error(err);
      const std::string report = mic::kraken::format_report(classifier->abundance_counts(), kl, kraken_rank);
      FILE* f = fopen(kraken_report.c_str(), "wb");
      if (!f || fwrite(report.data(), 1, report.size(), f) != report.size() || fclose(f) != 0)
        throw std::runtime_error("Failed to write the Kraken report: " + kraken_report);
      std::cout << " - Kraken report stored in " << kraken_report << std::endl;
    }
    if (!density.empty()) {
      const std::vector<uint64_t> counts = classifier->density_counts();
      const std::string report = mic::density::format_report(counts.data());
      FILE* f = fopen(density.c_str(), "wb");
      if (!f || fwrite(report.data(), 1, report.size(), f) != report.size() || fclose(f) != 0)
        throw std::runtime_error("Failed to write the density report: " + density);
      std::cout << " - Density report stored in " << density << std::endl;
    }
    if (!kmer_report.empty()) {
      std::vector<uint8_t> regs;
      std::vector<uint64_t> hits;
      classifier->ksketch_result(regs, hits);
      const std::vector<uint64_t> ab = classifier->abundance_counts();
      const std::vector<std::string>& names = classifier->target_names();
      std::vector<const char*> nm(names.size());
      for (size_t t = 0; t < names.size(); ++t) nm[t] = names[t].c_str();
      const std::string report = mic::ksketch::format_report(nm.data(), ab.data() + 2, regs.data(), hits.data(), (uint32_t)names.size());
      FILE* f = fopen(kmer_report.c_str(), "wb");
      if (!f || fwrite(report.data(), 1, report.size(), f) != report.size() || fclose(f) != 0)
        throw std::runtime_error("Failed to write the k-mer report: " + kmer_report);
      std::cout << " - K-mer report stored in " << kmer_report << std::endl;
    }
    if (!kmer_coverage.empty()) {
      std::vector<uint8_t> regs;
      std::vector<uint64_t> hits;
      classifier->ksketch_result(regs, hits);
      const std::vector<uint64_t> ab = classifier->abundance_counts();
      const std::vector<uint64_t> tk = classifier->census_counts();
      const std::vector<std::string>& names = classifier->target_names();
      std::vector<const char*> nm(names.size());
      for (size_t t = 0; t < names.size(); ++t) nm[t] = names[t].c_str();
      std::string report;
      uint32_t bad = 0;
      if (!mic::ksketch::format_coverage(nm.data(), ab.data() + 2, regs.data(), hits.data(), tk.data(), (uint32_t)names.size(), report, &bad))
        throw std::runtime_error("--kmer-coverage: the objects hit k-mers of " + names[bad] + ", of which the table census counted none");
      FILE* f = fopen(kmer_coverage.c_str(), "wb");
      if (!f || fwrite(report.data(), 1, report.size(), f) != report.size() || fclose(f) != 0)
        throw std::runtime_error("Failed to write the k-mer coverage report: " + kmer_coverage);
      std::cout << " - K-mer coverage report stored in " << kmer_coverage << std::endl;
    }
  } catch (const std::exception& ex) {
    std::cerr << ex.what() << std::endl;
    delete classifier;
    return 1;
  }
  // The results are written and closed.  Taking the engines apart in order - tens of gigabytes of table, staging and pinned slots
  // freed one allocation at a time - took the headline run a second (4.46 s of process for 3.45 s of work); the process ends here and
  // the driver takes everything back at once.  MIC_CLI_ORDERLY_EXIT=1 keeps the orderly teardown (the sanitizer builds run with it).
  std::cout.flush(); std::cerr.flush();
  fflush(nullptr);
  // (under a profiler or a coverage / trace tool - rocprofv3 preloads its library and flushes its output from an exit handler - the
  // orderly road is taken without being asked: a fast exit would lose the tool's output)
  auto tooled = [] {
    for (const char* v : {"ROCP_TOOL_LIBRARIES", "ROCPROFILER_REGISTER_FORCE_LOAD", "HSA_TOOLS_LIB", "LLVM_PROFILE_FILE"}) if (getenv(v)) return true;
    const char* pre = getenv("LD_PRELOAD");
    return pre && (strstr(pre, "rocprof") || strstr(pre, "roctracer") || strstr(pre, "guardalloc"));      // (sanitizer runs ask with the variable)
  };
  if (!getenv("MIC_CLI_ORDERLY_EXIT") && !tooled()) _exit(0);
  delete classifier;
  return 0;
}
