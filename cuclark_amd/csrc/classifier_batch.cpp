// classifier_batch.cpp - the batch path of the command line, the reference's own flow per input segment: index the reads
// (CuCLARK_hh.hh:1339-1534), pack them into the engine's lent buffers (:1616-1716), mic_batch_query / wait (queryBatch / waitForBatch),
// format the CSV lines (:1951-2139), write in order.  Used for --extended, for batches the device path hands back, and with
// MIC_HOST_INGEST=1.
#include "classifier_internal.hpp"

namespace mic {
using namespace detail;

void Classifier::release_batches() {
  for (mic_engine* e : engines_) mic_batches_free(e);
  lent_.clear();
  slot_reads_ = slot_cont_ = 0;
}

// batch slots are allocated once and reused by every segment; they grow when a segment needs more
void Classifier::ensure_batches(size_t max_reads, size_t max_cont) {
  if (!lent_.empty() && max_reads <= slot_reads_ && max_cont <= slot_cont_) return;
  release_batches();
  const size_t n_eng = engines_.size();
  slots_per_engine_ = std::max<size_t>(1, (opt_.batches + groups_ - 1) / groups_);
  slot_reads_ = max_reads + max_reads / 8 + 64;
  slot_cont_ = max_cont + max_cont / 8 + 64;
  row_words_ = (opt_.extended || ranking()) ? (uint32_t)std::min<size_t>(names_.size() + 1, 65) : 16;
  lent_.resize(n_eng);
  std::vector<uint32_t> index(slots_per_engine_ + 1);
  for (size_t i = 0; i <= slots_per_engine_; ++i) index[i] = (uint32_t)(i * slot_reads_);   // fixed stride: slot i owns rows [i*S, (i+1)*S)
  for (size_t d = 0; d < n_eng; ++d) {
    Lent& L = lent_[d];
    L.rp.resize(slots_per_engine_); L.ct.resize(slots_per_engine_);
    check(mic_batches_alloc(engines_[d], slots_per_engine_ * slot_reads_, slot_reads_, slot_cont_, index.data(),
                            (opt_.extended || parts_ > 1 || ranking()) ? 1 : 0,
                            &L.results, &L.rows, L.rp.data(), L.ct.data()), "batch allocation");
  }
}

void Classifier::run_segments(SegmentSource& src, const std::string& results_base, bool paired) {
  const std::string csv = results_base + ".csv";  // CuCLARK_hh.hh:539-540
  csv_out_ = !results_base.empty();               // (no -R: a summary-only --abundance run writes no result CSV)
  FILE* fout = csv_out_ ? fopen(csv.c_str(), "w") : nullptr;
  if (csv_out_ && !fout) { std::cerr << "Failed to create/open file result: " << csv << std::endl; return; }
  // --classified-out / --unclassified-out: the two files, created even when they stay empty; process_segment appends in order
  const std::string* split_name[2] = {&opt_.classified_out, &opt_.unclassified_out};
  for (int c = 0; c < 2; ++c) {
    split_fd_[c] = -1;
    if (split_name[c]->empty()) continue;
    unlink(split_name[c]->c_str());
    split_fd_[c] = open(split_name[c]->c_str(), O_CREAT | O_WRONLY | O_TRUNC, 0644);
    if (split_fd_[c] == -1) { std::cerr << "Failed to create/open file: " << *split_name[c] << std::endl; if (fout) fclose(fout); if (c && split_fd_[0] != -1) { close(split_fd_[0]); split_fd_[0] = -1; } return; }
  }
  // --hit-maps: the file with its header line; process_segment appends every segment's text in order
  hitmap_fd_ = -1;
  if (mapping()) {
    unlink(map_file().c_str());
    hitmap_fd_ = open(map_file().c_str(), O_CREAT | O_WRONLY | O_TRUNC, 0644);
    const size_t hl = strlen(map_header());      // (--kraken-out: no header line)
    if (hitmap_fd_ == -1 || write(hitmap_fd_, map_header(), hl) != (ssize_t)hl) {
      std::cerr << "Failed to create/open file: " << map_file() << std::endl;
      if (hitmap_fd_ != -1) { close(hitmap_fd_); hitmap_fd_ = -1; }
      if (fout) fclose(fout);
      for (int c = 0; c < 2; ++c) if (split_fd_[c] != -1) { close(split_fd_[c]); split_fd_[c] = -1; }
      return;
    }
  }
  reset_counts();
  struct timeval t0, t1;
  gettimeofday(&t0, nullptr);
  n_objects_ = 0;
  if (fout) {  // header (CuCLARK_hh.hh:1957-1972)
    std::vector<const char*> nm(names_.size());
    size_t cap = 256;
    for (size_t t = 0; t < names_.size(); ++t) { nm[t] = names_[t].c_str(); cap += names_[t].size() + 2; }
    std::vector<char> hb(cap);
    int w = mic_csv_header(hb.data(), hb.size(), opt_.extended ? 1 : 0, nm.data(), (uint32_t)names_.size());
    if (w > 0 && fwrite(hb.data(), 1, (size_t)w, fout) != (size_t)w) { fclose(fout); die("cannot write " + csv + " (disk full?)"); }
  }
  // double buffering: segment i+1 is produced on a side thread while segment i is classified
  Segment cur, nxt;
  bool have = src.next(cur);
  std::string err;
  while (have) {
    bool have_next = false;
    std::string reader_err;
    std::thread reader([&] {
      try { have_next = src.next(nxt); } catch (const std::exception& ex) { reader_err = ex.what(); }
    });
    try { n_objects_ += process_segment(cur.p, cur.n, paired, fout); } catch (const std::exception& ex) { if (err.empty()) err = ex.what(); }
    reader.join();
    if (err.empty() && !reader_err.empty()) err = reader_err;
    if (!err.empty()) break;
    std::swap(cur, nxt);
    if (!cur.own.empty()) cur.p = (const uint8_t*)cur.own.data();
    nxt = Segment();
    have = have_next;
  }
  // a full disk shows here at the latest (the command line leaves through _exit: nothing later would flush or report it)
  const bool write_failed = fout && ferror(fout) != 0;
  if (fout && (fclose(fout) != 0 || write_failed)) { if (err.empty()) err = "cannot write " + csv + " (disk full?)"; }
  for (int c = 0; c < 2; ++c)
    if (split_fd_[c] != -1) { if (close(split_fd_[c]) != 0 && err.empty()) err = "cannot write " + *split_name[c] + " (disk full?)"; split_fd_[c] = -1; }
  if (hitmap_fd_ != -1) { if (close(hitmap_fd_) != 0 && err.empty()) err = "cannot write " + map_file() + " (disk full?)"; hitmap_fd_ = -1; }
  release_batches();
  if (!err.empty()) die(err);
  gettimeofday(&t1, nullptr);
  const double diff = (t1.tv_sec - t0.tv_sec) + (t1.tv_usec - t0.tv_usec) / 1000000.0;
  std::cout << " - Assignment time: " << diff << " s. Speed: ";  // CuCLARK_hh.hh:1938-1944
  std::cout << (size_t)(((double)n_objects_) / (diff) * 60.0) << " objects/min. (" << n_objects_ << " objects)." << std::endl;
  if (csv_out_) std::cout << " - Results stored in " << csv << std::endl;
}

size_t Classifier::process_segment(const uint8_t* map, size_t nb, bool paired, FILE* fout) {
  struct timeval t0;
  gettimeofday(&t0, nullptr);
  const bool timing = getenv("MIC_CLI_TIMING") != nullptr;
  double last = 0;
  auto lap = [&](const char* what) {
    if (!timing) return;
    struct timeval t; gettimeofday(&t, nullptr);
    double now = (t.tv_sec - t0.tv_sec) + (t.tv_usec - t0.tv_usec) / 1e6;
    std::cerr << "[timing] " << what << ": " << (now - last) << " s" << std::endl;
    last = now;
  };
  // ---- index (CuCLARK_hh.hh:1339-1534)
  if (nb == 0 || (map[0] != '>' && map[0] != '@')) { std::cerr << "Failed to recognize the format of the file." << std::endl; exit(-1); }
  // --min-base-quality: what is classified on the host is masked on the host, by the same rule (mic_qmask.h) - a copy of the FASTQ
  // text with 'N' for every masked base; merged pairs arrive masked (they are FASTA text)
  const uint8_t* const original = map;        // (--classified-out / --unclassified-out copy the records as they came, whatever is masked)
  std::vector<uint8_t> masked;
  if (opt_.min_quality_byte && map[0] == '@') {
    masked.resize(nb);
    if (mic_fastq_mask_quality(map, nb, opt_.min_quality_byte, masked.data()) != MIC_OK)
      die("--min-base-quality needs FASTQ records of four lines each (the input's line count is no multiple of four).");
    map = masked.data();
  }
  // --mask-low-complexity: the same for the rule of mic_lowc.h, once per segment and after the quality mask (FASTA, merged pairs
  // included, and FASTQ); the device never rewrites a text, so a batch it hands back arrives here unmasked
  if (opt_.low_complexity) {
    if (masked.empty()) masked.assign(map, map + nb);
    if (mic_text_mask_low_complexity(masked.data(), nb, opt_.low_complexity, masked.data()) != MIC_OK) die("--mask-low-complexity: the text could not be masked.");
    map = masked.data();
  }
  size_t cap = std::max<size_t>(1024, nb / 96);
  // index arrays live across segments: resizing a fresh vector zero-fills ~200 MB per 512 MB segment
  std::vector<uint64_t>&name_s = ix_[0], &name_e = ix_[1], &seq_s = ix_[2], &seq_e = ix_[3], &length = ix_[4];
  if (name_s.size() > cap) cap = name_s.size();
  long n_reads;
  for (;;) {
    if (name_s.size() < cap) { name_s.resize(cap); name_e.resize(cap); seq_s.resize(cap); seq_e.resize(cap); length.resize(cap); }
    n_reads = mic_index_reads_parallel(map, nb, sink_ ? 1 : (int)opt_.threads, cap, name_s.data(), name_e.data(), seq_s.data(), seq_e.data(),
                                       length.data());
    if (n_reads < 0) { std::cerr << "Failed to recognize the format of the file." << std::endl; exit(-1); }
    if ((size_t)n_reads <= cap) break;
    cap = (size_t)n_reads;
  }
  const size_t N = (size_t)n_reads;
  lap("index reads");
  const int k = (int)opt_.k;
  // A batch the streaming path hands back (sink_ set) is small and comes while that path's loader / device / writer threads are
  // running: no OpenMP team for it - a team's idle threads spin at the barriers and between the regions (libgomp's default wait
  // policy), and next to the stream's threads that spinning ran a 64-read batch into 0.2-0.5 s of cgroup throttling
  // (tools/cli_small_slots_probe.py: 55 such batches 14.2 s, 0.6 s with OMP_WAIT_POLICY=PASSIVE).
  const int team = sink_ ? 1 : (int)std::max<size_t>(1, opt_.threads);
  const size_t nb_total = std::max<size_t>(1, std::min(opt_.batches, std::max<size_t>(N, 1)));
  const size_t per = (N + nb_total - 1) / nb_total;
  std::vector<size_t> cut(nb_total + 1);
  for (size_t b = 0; b <= nb_total; ++b) cut[b] = std::min(N, b * per);
  size_t max_reads = 0, max_cont = 0;
  {
    std::vector<size_t> bound(nb_total);
#ifdef _OPENMP
#pragma omp parallel for schedule(static) num_threads(team)
#endif
    for (long b = 0; b < (long)nb_total; ++b)
      bound[b] = mic_pack_bound(seq_s.data() + cut[b], seq_e.data() + cut[b], cut[b + 1] - cut[b], k);
    for (size_t b = 0; b < nb_total; ++b) {
      max_reads = std::max(max_reads, cut[b + 1] - cut[b]);
      max_cont = std::max(max_cont, bound[b]);
    }
  }
  ensure_batches(max_reads, max_cont);
  lap("batch slots");

  // ---- batches: pack -> query -> wait -> format; ordered write
  std::vector<std::string> out(nb_total);
  std::vector<std::string> hm_out(mapping() ? nb_total : 0);       // --hit-maps: every batch's text, written in the same order
  std::vector<char> ready(nb_total, 0);
  std::mutex wmu;
  size_t next_write = 0;
  std::string err;
  const uint32_t T = (uint32_t)names_.size();
  std::vector<const char*> nm(names_.size());
  for (size_t t = 0; t < names_.size(); ++t) nm[t] = names_[t].c_str();
  const uint32_t row_words = row_words_;
  const size_t line_cap = 512 + (opt_.extended ? (size_t)T * 12 : 0);

  // --classified-out / --unclassified-out: every read's result row as the CSV shows it and its Length column, for mic_split_host below
  const int split = paired ? 0 : splitting();
  std::vector<uint32_t> sp_res(split ? N * MIC_RESULT_WORDS : 0), sp_norm(split ? N : 0);
  double t_pack = 0, t_query = 0, t_format = 0, t_write = 0;   // thread-seconds, MIC_CLI_TIMING only
  auto now_s = [] { struct timeval t; gettimeofday(&t, nullptr); return t.tv_sec + t.tv_usec / 1e6; };
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic) reduction(+ : t_pack, t_query, t_format, t_write) num_threads(team)
#endif
  for (long bi = 0; bi < (long)nb_total; ++bi) {
    double ts = timing ? now_s() : 0;
    auto tick = [&](double& acc) { if (timing) { const double n = now_s(); acc += n - ts; ts = n; } };
    // batch b belongs to read group b % groups_: one engine (table replicated), or the parts_ engines that hold the table's parts
    const bool sharded = parts_ > 1;
    const size_t b = (size_t)bi, grp = b % groups_, d = grp * parts_, lb = b / groups_;
    mic_engine* const* group = engines_.data() + d;
    Lent& L = lent_[d];
    const size_t r0 = cut[b], cnt = cut[b + 1] - cut[b];
    try {
      size_t m = mic_pack_reads(map, seq_s.data() + r0, seq_e.data() + r0, length.data() + r0, cnt, k, L.rp[lb], L.ct[lb], slot_cont_);
      if (m == (size_t)-1) die("ERROR: Batch overflow. Please increase the number of batches (-b <numberofbatches>).");
      tick(t_pack);
      if (!sharded) {
        check(mic_batch_ready(engines_[d], lb, cnt, m), "readyBatch");
        check(mic_batch_query(engines_[d], lb, (opt_.extended || ranking()) ? 1 : 0, 0), "queryBatch");
        check(mic_batch_wait(engines_[d], lb), "waitForBatch");
        if (sketching()) check(mic_batch_ksketch(engines_[d], lb), "k-mer sketches");      // (the batch's packed reads and results are still on the device)
        if (mapping()) {     // likewise: the maps of the batch's reads (sized, then fetched), as text with the names this path has
          uint64_t nw = 0;
          std::vector<uint32_t> hm_off(cnt + 1, 0), hm_words;
          check(mic_batch_hitmap(engines_[d], lb, hm_off.data(), hm_off.size(), nullptr, 0, &nw), "hit maps");
          hm_words.resize((size_t)nw);
          if (nw) check(mic_batch_hitmap(engines_[d], lb, hm_off.data(), hm_off.size(), hm_words.data(), hm_words.size(), &nw), "hit maps");
          std::vector<std::string> rn(cnt);
          std::vector<const char*> rnp(cnt);
          for (size_t i = 0; i < cnt; ++i) { rn[i].assign((const char*)map + name_s[r0 + i], (size_t)(name_e[r0 + i] - name_s[r0 + i])); rnp[i] = rn[i].c_str(); }
          // --kraken-out: the same words under the batch's result rows and Length column (mic_kraken.h), no new device call
          std::vector<uint32_t> kr_norm(kraken() ? cnt : 0);
          for (size_t i = 0; i < kr_norm.size(); ++i) kr_norm[i] = (uint32_t)(paired ? length[r0 + i] - 1 : length[r0 + i]);
          const uint32_t* kr_res = L.results + lb * slot_reads_ * MIC_RESULT_WORDS;
          auto format = [&](char* buf, size_t cap) {
            return kraken() ? mic_kraken_format(rnp.data(), cnt, kr_res, kr_norm.data(), k, T, &opt_.abund_filter, hm_off.data(), hm_words.data(), nm.data(), buf, cap)
                            : mic_hitmap_format(rnp.data(), cnt, hm_off.data(), hm_words.data(), nm.data(), T, buf, cap);
          };
          const long len = format(nullptr, 0);
          if (len < 0) die("hit maps: the text could not be formatted");
          std::string& ht = hm_out[b];
          ht.resize((size_t)len + 1);
          if (format(&ht[0], ht.size()) != len) die("hit maps: the text could not be formatted");
          ht.resize((size_t)len);
        }
      } else {
        // every engine of the group probes the same reads against its part of the table - one upload into the first engine, the packed
        // reads fanned out device to device (mic_batch_query_group; the reference uploads the host arrays to every device,
        // CuClarkDB.cu:886-890) - and the rows are summed read-range owned into the first engine's host arrays (mic_batch_merge_shards)
        check(mic_batch_ready(group[0], lb, cnt, m), "readyBatch");
        check(mic_batch_query_group(group, parts_, lb, 1), "queryBatch");
        check(mic_batch_merge_shards(group, parts_, lb), "merge of the table shards");
      }
      tick(t_query);
      std::string& s = out[b];
      const bool emit = csv_out_;
      if (emit) s.reserve(cnt * (opt_.extended ? 64 + 3 * (size_t)T : 72));
      std::vector<char> line(line_cap);
      std::vector<uint32_t> dense;
      std::vector<uint32_t> ab_res, ab_norm;        // --abundance: the batch's result rows as the CSV shows them, and the Length column
      if (counting() || densing()) ab_res.resize(cnt * MIC_RESULT_WORDS);
      if (counting() || ranking() || densing()) ab_norm.resize(cnt);
      // --rank-report: this batch's roll-up counters, from its sparse rows and - a read at a time - the dense counts of the rows that did not fit
      std::vector<uint64_t> ru_counts(ranking() ? lineage_.n_counters() : 0, 0);
      const uint32_t* res = L.results + lb * slot_reads_ * MIC_RESULT_WORDS;
      const uint32_t* rows = L.rows ? L.rows + lb * slot_reads_ * row_words : nullptr;
      for (size_t i = 0; i < cnt; ++i) {
        const size_t r = r0 + i;
        const uint32_t* row = rows ? rows + i * row_words : nullptr;
        const uint32_t* dn = nullptr;
        const uint32_t* rr = res + i * MIC_RESULT_WORDS;
        uint32_t fixed[MIC_RESULT_WORDS];
        if (row && row[0] == MIC_ROW_INVALID) {
          dense.resize(T);
          if (!sharded) {
            check(mic_batch_dense_counts(engines_[d], lb, i, dense.data()), "dense counts");
          } else {
            // more targets than a sparse row holds: dense counts of every shard, summed; best / second-best under the
            // reference's order (count descending, target ascending)
            std::vector<uint32_t> part(T);
            std::fill(dense.begin(), dense.end(), 0u);
            for (size_t g = 0; g < parts_; ++g) {
              check(mic_batch_dense_counts(group[g], lb, i, part.data()), "dense counts");
              for (uint32_t t2 = 0; t2 < T; ++t2) dense[t2] += part[t2];
            }
            uint32_t sum = 0, best = 0, ib = 0, sb = 0, is = 0, hit = 0;
            for (uint32_t t2 = 0; t2 < T; ++t2) {
              const uint32_t sc = dense[t2];
              if (!sc) continue;
              ++hit; sum += sc;
              if (sc > best) { sb = best; is = ib; best = sc; ib = t2 + 1; }
              else if (sc > sb) { sb = sc; is = t2 + 1; }
            }
            fixed[0] = sum; fixed[1] = ib; fixed[2] = best; fixed[3] = is; fixed[4] = sb; fixed[5] = hit; fixed[6] = rr[6]; fixed[7] = 0;
            rr = fixed;
          }
          dn = dense.data();
        }
        if (split) { memcpy(&sp_res[r * MIC_RESULT_WORDS], rr, MIC_RESULT_WORDS * 4); sp_norm[r] = (uint32_t)length[r]; }
        if (counting() || densing()) memcpy(&ab_res[i * MIC_RESULT_WORDS], rr, MIC_RESULT_WORDS * 4);
        if (counting() || ranking() || densing()) ab_norm[i] = (uint32_t)(paired ? length[r] - 1 : length[r]);      // (the CSV's Length column, CuCLARK_hh.hh:2119)
        if (ranking() && dn)
          check(mic_rollup_host(nullptr, 0, dn, &ab_norm[i], 1, k, T, lineage_.n_levels, lineage_.group_of.data(), &opt_.abund_filter, nullptr, nullptr,
                                ru_counts.data()), "roll-up (host path, dense counts)");
        if (!emit) continue;
        int w = mic_csv_line(line.data(), line.size(), map + name_s[r], (size_t)(name_e[r] - name_s[r]), length[r], paired ? 1 : 0,
                             k, rr, nm.data(), T, opt_.extended ? 1 : 0, row, dn);
        if (w < 0) die("CSV line too long");
        s.append(line.data(), (size_t)w);
      }
      if (counting() || densing()) count_host(ab_res, ab_norm);       // (--abundance and --density: each counts its own)
      if (ranking()) {
        check(mic_rollup_host(rows, row_words, nullptr, ab_norm.data(), cnt, k, T, lineage_.n_levels, lineage_.group_of.data(), &opt_.abund_filter,
                              nullptr, nullptr, ru_counts.data()), "roll-up (host path)");
        std::lock_guard<std::mutex> lk(count_mu_);
        if (host_rollup_.size() != ru_counts.size()) host_rollup_.assign(ru_counts.size(), 0);
        for (size_t j = 0; j < ru_counts.size(); ++j) host_rollup_[j] += ru_counts[j];
      }
    } catch (const std::exception& ex) {
      std::lock_guard<std::mutex> lk(wmu);
      if (err.empty()) err = ex.what();
    }
    tick(t_format);
    std::lock_guard<std::mutex> lk(wmu);
    ready[b] = 1;
    while (next_write < nb_total && ready[next_write]) {
      if (sink_) sink_->append(out[next_write]);
      else if (fout && fwrite(out[next_write].data(), 1, out[next_write].size(), fout) != out[next_write].size() && err.empty()) err = "short write to the result file (disk full?)";
      std::string().swap(out[next_write]);
      if (mapping()) {
        std::string& ht = hm_out[next_write];
        if (sink_) { if (hitmap_sink_) hitmap_sink_->append(ht); }
        else for (size_t done = 0; done < ht.size() && err.empty();) {
          const ssize_t w = write(hitmap_fd_, ht.data() + done, ht.size() - done);
          if (w <= 0) { err = "cannot write " + map_file() + " (disk full?)"; break; }
          done += (size_t)w;
        }
        std::string().swap(ht);
      }
      ++next_write;
    }
    tick(t_write);
  }
  lap("pack + query + format + write");
  if (timing)
    std::cerr << "[timing]   thread-seconds: pack " << t_pack << ", copy+query+wait " << t_query << ", format " << t_format
              << ", ordered write " << t_write << std::endl;
  if (!err.empty()) die(err);
  if (split) {       // the segment's ORIGINAL bytes, cut at the host indexer's records (mic_split.h)
    std::vector<uint64_t> start(N);
    for (size_t r = 0; r < N; ++r) start[r] = name_s[r] - 1;
    std::vector<uint8_t> part(nb + 1);
    uint64_t tot[4] = {0, 0, 0, 0};
    if (mic_split_host(original, nb, start.data(), N, sp_res.data(), sp_norm.data(), k, T, &opt_.abund_filter, split, part.data(), tot) != MIC_OK)
      die("--classified-out / --unclassified-out: the records of the input do not tile it (a record the reader does not take as it is).");
    const uint8_t* piece[2] = {part.data(), part.data() + tot[0]};
    for (int c = 0; c < 2; ++c) {
      if (!(split & (1 << c))) continue;
      const size_t n = (size_t)tot[c];
      if (sink_) { if (split_sink_[c]) split_sink_[c]->append((const char*)piece[c], n); continue; }
      for (size_t done = 0; done < n;) {
        const ssize_t w = write(split_fd_[c], piece[c] + done, n - done);
        if (w <= 0) die("cannot write " + (c ? opt_.unclassified_out : opt_.classified_out) + " (disk full?)");
        done += (size_t)w;
      }
    }
  }
  return N;
}

}  // namespace mic
