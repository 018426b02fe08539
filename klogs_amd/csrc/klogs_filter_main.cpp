// klogs-filter — the klogs batch path (rootCmd.Run, /root/reference/cmd/root.go:442-474)
// over captured log bodies, with the filter on the GPU through libklf.
//
//   klogs-filter [-p logpath] [-s since] [-t tail] [-i] [--grep LIT]... [--match RE]...
//                [-A N] [-B N] [-C N] [--invert-match] [--from X] [--until X] [--histogram WIDTH]
//                [--around D] [--around-before D] [--around-after D]
//                [--record-indent] [--record-blank] [--record-cont PREFIX]... [--record-head PREFIX]...
//                [--record-invert]
//                [--merge [--merge-timestamps]] [--top K [--top-mask-digits] [--top-key-bytes N]]
//                [--stat KEY [--stat-decimals D | --stat-duration]]
//                [--now UNIX_SEC[.NSEC]] [--device N] [--no-color] MANIFEST
//
// -A / -B / -C N (lines of context after / before / around a matching line) and
// --invert-match (the lines that do not match) need a --grep or --match; they are grep's,
// not the reference's (-v stays its version flag): SPEC.md S4a, klf_regroup.
//
// --from X / --until X keep the lines whose timestamp lies in [from, until) (SPEC.md S4b,
// klf_window), before --since and --tail apply: X is an RFC3339Nano instant or a Go duration
// meaning that long before --now.  They work with and without a pattern and combine with the
// context flags in one call.
//
// --around D keeps every line, of every container, whose timestamp lies within D of a matching
// line of any container (SPEC.md S4g, klf_around): what the others were doing when it happened.
// D is a Go duration >= 0 and at most 2^62 - 1 ns; --around-before D / --around-after D set the
// reach ahead of / behind a match alone and override --around.  They need a --grep or --match,
// exclude -A / -B / -C / --invert-match, and combine with --from / --until (the cut is made
// after the context is taken), --since, --tail, --merge, --histogram, --top and --stat.
//
// --record-* select whole multi-line records (SPEC.md S4h, klf_records): a stack trace, a panic
// dump or a traceback goes out with the line that matched, and nothing behind it does.  A record
// is a head line and the continuation lines behind it.  A line continues a record when it begins
// with a space or a tab (--record-indent), is empty (--record-blank) or begins with a --record-cont
// PREFIX; or, with --record-head PREFIX given, when it begins with none of them (the other three
// are then refused).  Up to 8 prefixes of 1..32 bytes.  --record-invert keeps the records without
// a match.  Any of the flags turns the stage on.  They need a --grep or --match, exclude -A / -B /
// -C / --invert-match / --around*, and combine with --from / --until (the cut is made after the
// records are taken), --since, --tail, --merge, --histogram, --top and --stat.
//
// --histogram WIDTH (a Go duration > 0) also writes <logpath>/histogram.tsv: per stream, the
// lines of the selection (after the pattern, the context flags and the window; before --since
// and --tail, SPEC.md S4c, klf_result_histogram) counted in buckets of WIDTH from --from (else
// the --since instant; one of the two is needed) up to --until (else --now), at most 65536.
//
// --merge also writes <logpath>/merged.log: the emitted lines of all containers in one
// chronological sequence (SPEC.md S4d, klf_result_timeline), each behind "<pod>/<container> ";
// --merge-timestamps keeps each line's timestamp.  The per-container files stay as they are.
//
// --top K (1..65536) also writes <logpath>/top.tsv: the K most frequent messages of the selection
// (after the pattern, the context flags and the window; before --since and --tail, SPEC.md S4e,
// klf_result_groups) over all containers, with their line counts and their first and last line.
// --top-mask-digits counts messages that differ only in their numbers as one (each run of
// digits shows as '#'); --top-key-bytes N compares the first N bytes of a message only.
//
// --stat KEY (1..64 bytes) also writes <logpath>/stats.tsv: the statistics of the number behind
// the first KEY of each line of the selection (after the pattern, the context flags and the
// window; before --since and --tail, SPEC.md S4f, klf_result_field_stats), one row per container
// and one over all of them ("*"): pod, container, lines, hits, bad, min, max, sum, p50, p90, p99
// and max_at = <pod>/<container>:<line, counted from 1> of the first line with the maximum; no
// header; "-" from min on without a hit.  --stat-decimals D (0..9) keeps D fraction digits;
// --stat-duration reads Go durations ("1m30.5s") and prints nanoseconds.
//
// MANIFEST has one line per container of the pod selection, in pod-spec order:
//   <pod> TAB <init|container> TAB <container> TAB <path of the captured body | ->
// A body is what GetLogs(...).Stream() returns for Timestamps=true without
// SinceSeconds/TailLines; "-" or an unreadable path is a failed Stream() call (:326-328:
// error line, the file stays empty).  Cluster discovery (:449-461) is out of scope: the
// manifest stands for its result.
#include <fcntl.h>
#include <sys/stat.h>
#include <time.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/klf.h"
#include "../../include/klogs_host.h"

namespace {

struct PodEnt {
  std::string name;
  std::vector<std::string> init, containers;
  std::vector<std::string> init_body, cont_body;
};

[[noreturn]] void panic_exit(const std::string& m) {
  std::fprintf(stderr, "panic: %s\n", m.c_str());
  std::exit(2);
}

bool read_file(const std::string& path, std::vector<uint8_t>& out) {
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) return false;
  out.clear();
  uint8_t buf[1 << 16];
  size_t n;
  while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) out.insert(out.end(), buf, buf + n);
  const bool ok = !std::ferror(f);
  std::fclose(f);
  return ok;
}

void usage() {
  std::fprintf(stderr,
               "usage: klogs-filter [-p logpath] [-s since] [-t tail] [-i] [--grep LIT]... [--match RE]...\n"
               "                    [-A N] [-B N] [-C N] [--invert-match]   (with --grep / --match: lines of\n"
               "                    context after / before / around a match; the lines that do not match)\n"
               "                    [--from X] [--until X]   (the lines with from <= timestamp < until, before\n"
               "                    --since / --tail apply; X: an RFC3339Nano instant, or a duration before --now)\n"
               "                    [--around D] [--around-before D] [--around-after D]   (with --grep / --match:\n"
               "                    the lines of every container within D, a duration >= 0, of a matching line of\n"
               "                    any container; ahead of / behind a match alone; not with -A / -B / -C /\n"
               "                    --invert-match)\n"
               "                    [--record-indent] [--record-blank] [--record-cont PREFIX]... [--record-head PREFIX]...\n"
               "                    [--record-invert]   (with --grep / --match: whole multi-line records, a head\n"
               "                    line and the lines behind it that begin with a space or tab / are empty / begin\n"
               "                    with PREFIX; or, with --record-head, that begin with none of its PREFIXes; the\n"
               "                    records without a match; up to 8 prefixes of 1..32 bytes; not with -A / -B / -C /\n"
               "                    --invert-match / --around*)\n"
               "                    [--histogram WIDTH]   (also writes <logpath>/histogram.tsv: the selected lines\n"
               "                    per stream in buckets of WIDTH, a duration > 0, from --from (else the --since\n"
               "                    instant; one of them is needed) up to --until (else --now), at most 65536\n"
               "                    buckets; counted before --since / --tail apply)\n"
               "                    [--merge [--merge-timestamps]]   (also writes <logpath>/merged.log: the emitted\n"
               "                    lines of all containers by time, each behind \"<pod>/<container> \"; with their\n"
               "                    timestamps)\n"
               "                    [--top K [--top-mask-digits] [--top-key-bytes N]]   (also writes <logpath>/top.tsv:\n"
               "                    the K most frequent messages of the selected lines, K in 1..65536, over all\n"
               "                    containers; with each run of digits counted as '#'; comparing the first N\n"
               "                    bytes of a message only; counted before --since / --tail apply)\n"
               "                    [--stat KEY [--stat-decimals D | --stat-duration]]   (also writes\n"
               "                    <logpath>/stats.tsv: per container and over all, the lines with the number\n"
               "                    behind KEY (1..64 bytes), their min, max, sum, p50, p90, p99 and where the\n"
               "                    maximum is; with D = 0..9 fraction digits kept; as Go durations, in ns;\n"
               "                    counted before --since / --tail apply)\n"
               "                    [--now UNIX_SEC[.NSEC]] [--device N] [--no-color] MANIFEST\n");
  std::exit(1);
}

}  // namespace

int main(int argc, char** argv) {
  std::string logpath, since, manifest;
  int64_t tail = -1;
  bool init = false, color = true;
  int device = 0;
  klf_time now{(int64_t)time(nullptr), 0, 0};
  std::vector<std::string> greps, matches;
  klf_regroup_opts regroup{0, 0, 0, 0};
  bool regrouped = false;  // any of -A / -B / -C / --invert-match
  std::string from_arg, until_arg;
  bool from_set = false, until_set = false;  // --from / --until
  std::string around_arg, around_before_arg, around_after_arg;
  bool around_set = false, around_before_set = false, around_after_set = false;  // --around, -before, -after
  uint32_t record_flags = 0;  // --record-indent, --record-blank, --record-invert
  std::vector<std::string> record_cont, record_head;  // --record-cont, --record-head
  bool recorded = false;  // any --record-*
  std::string hist_arg;
  bool hist_set = false;  // --histogram
  bool merge = false, merge_ts = false;  // --merge, --merge-timestamps
  klf_groups_opts top{0, 0, 0, 0};
  bool top_set = false, top_mask = false, top_key_set = false;  // --top, --top-mask-digits, --top-key-bytes
  std::string stat_key;
  uint32_t stat_decimals = 0;
  bool stat_set = false, stat_dec_set = false, stat_duration = false;  // --stat, --stat-decimals, --stat-duration
  auto number = [&](const std::string& v, unsigned long long max) -> uint32_t {
    char* end = nullptr;
    const unsigned long long x = std::strtoull(v.c_str(), &end, 10);
    if (v.empty() || v[0] < '0' || v[0] > '9' || *end || x > max) usage();
    return (uint32_t)x;
  };
  auto context = [&](const std::string& v) -> uint32_t {
    char* end = nullptr;
    const unsigned long long x = std::strtoull(v.c_str(), &end, 10);
    if (v.empty() || v[0] == '-' || *end) usage();
    regrouped = true;
    return x > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)x;
  };
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    auto val = [&]() -> std::string {
      if (i + 1 >= argc) usage();
      return argv[++i];
    };
    if (a == "-p" || a == "--logpath") logpath = val();
    else if (a == "-s" || a == "--since") since = val();
    else if (a == "-t" || a == "--tail") tail = std::strtoll(val().c_str(), nullptr, 10);
    else if (a == "-i" || a == "--init") init = true;
    else if (a == "--grep") greps.push_back(val());
    else if (a == "--match") matches.push_back(val());
    else if (a == "-A" || a == "--after-context") regroup.after = context(val());
    else if (a == "-B" || a == "--before-context") regroup.before = context(val());
    else if (a == "-C" || a == "--context") regroup.before = regroup.after = context(val());
    else if (a == "--invert-match") { regroup.flags |= KLF_REGROUP_INVERT; regrouped = true; }
    else if (a == "--from") { from_arg = val(); from_set = true; }
    else if (a == "--until") { until_arg = val(); until_set = true; }
    else if (a == "--around") { around_arg = val(); around_set = true; }
    else if (a == "--around-before") { around_before_arg = val(); around_before_set = true; }
    else if (a == "--around-after") { around_after_arg = val(); around_after_set = true; }
    else if (a == "--record-indent") { record_flags |= KLF_RECORDS_INDENT; recorded = true; }
    else if (a == "--record-blank") { record_flags |= KLF_RECORDS_BLANK; recorded = true; }
    else if (a == "--record-invert") { record_flags |= KLF_RECORDS_INVERT; recorded = true; }
    else if (a == "--record-cont") { record_cont.push_back(val()); recorded = true; }
    else if (a == "--record-head") { record_head.push_back(val()); recorded = true; }
    else if (a == "--histogram") { hist_arg = val(); hist_set = true; }
    else if (a == "--merge") merge = true;
    else if (a == "--merge-timestamps") merge_ts = true;
    else if (a == "--top") { top.top = number(val(), KLF_GROUPS_MAX_TOP); top_set = true; }
    else if (a == "--top-mask-digits") top_mask = true;
    else if (a == "--top-key-bytes") { top.max_key = number(val(), 0xFFFFFFFFull); top_key_set = true; }
    else if (a == "--stat") { stat_key = val(); stat_set = true; }
    else if (a == "--stat-decimals") { stat_decimals = number(val(), 9); stat_dec_set = true; }
    else if (a == "--stat-duration") stat_duration = true;
    else if (a == "--device") device = std::atoi(val().c_str());
    else if (a == "--no-color") color = false;
    else if (a == "--now") {
      const std::string v = val();
      const size_t dot = v.find('.');
      now.sec = std::strtoll(v.substr(0, dot).c_str(), nullptr, 10);
      if (dot != std::string::npos) {
        std::string frac = v.substr(dot + 1);
        frac.resize(9, '0');
        now.nsec = (int32_t)std::strtol(frac.c_str(), nullptr, 10);
      }
    } else if (!a.empty() && a[0] == '-') usage();
    else manifest = a;
  }
  if (manifest.empty()) usage();
  if (regrouped && greps.empty() && matches.empty()) usage();  // context / inversion of what?
  const bool around = around_set || around_before_set || around_after_set;
  if (around && ((greps.empty() && matches.empty()) || regrouped)) usage();  // around what? / no line context with it
  if (recorded && ((greps.empty() && matches.empty()) || regrouped || around)) usage();  // records of what? / one transform a call
  if (!record_head.empty() && (!record_cont.empty() || (record_flags & (KLF_RECORDS_INDENT | KLF_RECORDS_BLANK)))) usage();
  if (merge_ts && !merge) usage();
  if ((top_set && top.top == 0) || ((top_mask || top_key_set) && !top_set)) usage();
  if (top_mask) top.flags |= KLF_GROUPS_MASK_DIGITS;
  if ((stat_set && (stat_key.empty() || stat_key.size() > KLF_FIELD_MAX_KEY)) || (stat_dec_set && stat_duration) ||
      ((stat_dec_set || stat_duration) && !stat_set))
    usage();
  // --from / --until: an instant, or a duration before `now` (--now may follow them)
  klf_window_opts window{{KLF_TIME_MIN_SEC, 0, 0}, {KLF_TIME_MAX_SEC, 0, 0},
                         regroup.before, regroup.after, regroup.flags, 0};
  auto bound = [&](const std::string& v, klf_time* t) {
    if (klf_parse_rfc3339nano((const uint8_t*)v.data(), v.size(), t) == 0) return;
    int64_t ns = 0;
    char perr[256];
    if (klh_parse_duration(v.c_str(), &ns, perr, sizeof(perr)) != KLH_OK) usage();
    int64_t sec = now.sec - ns / 1000000000, nsec = (int64_t)now.nsec - ns % 1000000000;
    if (nsec < 0) { nsec += 1000000000; --sec; }
    if (nsec >= 1000000000) { nsec -= 1000000000; ++sec; }
    *t = klf_time{sec, (int32_t)nsec, 0};
  };
  if (from_set) bound(from_arg, &window.from);
  if (until_set) bound(until_arg, &window.until);
  const bool windowed = from_set || until_set;
  // --around: both reaches, then each one's own flag; the bounds ride along
  klf_around_opts around_opts{window.from, window.until, 0, 0, 0, 0};
  auto reach = [&](const std::string& v) -> uint64_t {
    int64_t ns = 0;
    char perr[256];
    if (klh_parse_duration(v.c_str(), &ns, perr, sizeof(perr)) != KLH_OK || ns < 0 || (uint64_t)ns > KLF_AROUND_MAX_NS)
      usage();
    return (uint64_t)ns;
  };
  if (around_set) around_opts.before_ns = around_opts.after_ns = reach(around_arg);
  if (around_before_set) around_opts.before_ns = reach(around_before_arg);
  if (around_after_set) around_opts.after_ns = reach(around_after_arg);
  // --record-*: the prefixes of the one mode, concatenated; the bounds ride along
  const std::vector<std::string>& record_pre = record_head.empty() ? record_cont : record_head;
  if (record_pre.size() > KLF_RECORDS_MAX_PREFIXES) usage();
  std::string record_bytes;
  std::vector<uint32_t> record_off{0};
  for (const std::string& p : record_pre) {
    if (p.empty() || p.size() > KLF_RECORDS_MAX_PREFIX) usage();
    record_bytes += p;
    record_off.push_back((uint32_t)record_bytes.size());
  }
  const klf_records_opts records_opts{window.from, window.until,
                                      record_pre.empty() ? nullptr : (const uint8_t*)record_bytes.data(),
                                      record_pre.empty() ? nullptr : record_off.data(), (uint32_t)record_pre.size(),
                                      record_flags | (record_head.empty() ? 0u : KLF_RECORDS_PREFIX_HEAD)};
  if (logpath.empty()) {  // defaultLogPath (:47)
    char buf[128];
    klh_default_log_path(now.sec, buf, sizeof(buf));
    logpath = buf;
  }

  // getLopOpts (:201-221)
  klf_filter filter;
  int rejected = 0;
  char err[512] = {0};
  if (klh_lop_opts(since.c_str(), tail, now, &filter, &rejected, err, sizeof(err)) != KLH_OK) panic_exit(err);
  filter.flags |= KLF_FILTER_NO_TIMING;  // (the CLI reads no device timing)

  // --histogram: buckets of WIDTH over [--from, else the --since instant; --until, else now)
  klf_hist_opts hist{{0, 0, 0}, 0, 0, 0};
  if (hist_set) {
    int64_t w = 0;
    char perr[256];
    if (klh_parse_duration(hist_arg.c_str(), &w, perr, sizeof(perr)) != KLH_OK || w <= 0) usage();
    if (!from_set && since.empty()) usage();  // no lower edge
    const klf_time lo = from_set ? window.from : filter.since, hi = until_set ? window.until : now;
    const __int128 span = ((__int128)hi.sec - lo.sec) * 1000000000 + (hi.nsec - lo.nsec);
    if (span <= 0) usage();
    const __int128 nb = (span + w - 1) / w;
    if (nb > KLF_HIST_MAX_BUCKETS || nb * w > (__int128)INT64_MAX) usage();
    hist = klf_hist_opts{{lo.sec, lo.nsec, 0}, (uint64_t)w, (uint32_t)nb, 0};
  }

  // the pod selection, grouped by pod in first-appearance order
  std::vector<PodEnt> pods;
  {
    FILE* f = std::fopen(manifest.c_str(), "r");
    if (!f) panic_exit("open " + manifest + ": no such file");
    char line[8192];
    while (std::fgets(line, sizeof(line), f)) {
      std::string l(line);
      while (!l.empty() && (l.back() == '\n' || l.back() == '\r')) l.pop_back();
      if (l.empty() || l[0] == '#') continue;
      std::vector<std::string> col;
      size_t p = 0;
      for (;;) {
        const size_t q = l.find('\t', p);
        col.push_back(l.substr(p, q == std::string::npos ? std::string::npos : q - p));
        if (q == std::string::npos) break;
        p = q + 1;
      }
      if (col.size() != 4) panic_exit("manifest line needs 4 tab-separated fields: " + l);
      PodEnt* pe = nullptr;
      for (auto& x : pods)
        if (x.name == col[0]) pe = &x;
      if (!pe) {
        pods.push_back(PodEnt{col[0], {}, {}, {}, {}});
        pe = &pods.back();
      }
      if (col[1] == "init") { pe->init.push_back(col[2]); pe->init_body.push_back(col[3]); }
      else { pe->containers.push_back(col[2]); pe->cont_body.push_back(col[3]); }
    }
    std::fclose(f);
  }
  std::vector<std::vector<const char*>> ip(pods.size()), cp(pods.size());
  std::vector<klh_pod> kp(pods.size());
  for (size_t i = 0; i < pods.size(); ++i) {
    for (auto& s : pods[i].init) ip[i].push_back(s.c_str());
    for (auto& s : pods[i].containers) cp[i].push_back(s.c_str());
    kp[i] = klh_pod{pods[i].name.c_str(), (uint32_t)ip[i].size(), ip[i].data(), (uint32_t)cp[i].size(), cp[i].data()};
  }
  // getPodLogs (:224-277): stream table + createLogFile per stream
  uint32_t n = 0;
  klh_stream_table(kp.data(), (uint32_t)kp.size(), init ? 1 : 0, nullptr, 0, &n);
  std::vector<klh_stream> table(n);
  klh_stream_table(kp.data(), (uint32_t)kp.size(), init ? 1 : 0, table.data(), n, &n);
  std::vector<std::string> files(n), cname(n), body(n);
  for (uint32_t i = 0; i < n; ++i) {
    const PodEnt& pe = pods[table[i].pod];
    cname[i] = table[i].is_init ? pe.init[table[i].container] : pe.containers[table[i].container];
    body[i] = table[i].is_init ? pe.init_body[table[i].container] : pe.cont_body[table[i].container];
    char path[8192];
    if (klh_create_log_file(logpath.c_str(), pe.name.c_str(), cname[i].c_str(), path, sizeof(path)) != KLH_OK)
      panic_exit("create log file for " + pe.name + "/" + cname[i]);
    files[i] = path;
  }
  std::fprintf(stderr, "INFO  Found %zu Pod(s) %u Container(s)\n", pods.size(), n);

  if (n > 0 && rejected) {  // the API server refuses every request: error lines, empty files
    for (uint32_t i = 0; i < n; ++i)
      std::fprintf(stderr, "ERROR Error getting logs for container %s\n%s\n", cname[i].c_str(),
                   "the server rejected our request (invalid PodLogOptions)");
  } else if (n > 0) {
    std::vector<klf_pattern> pats;
    for (auto& g : greps) pats.push_back(klf_pattern{(const uint8_t*)g.data(), (uint32_t)g.size(), KLF_PAT_LITERAL});
    for (auto& m : matches) pats.push_back(klf_pattern{(const uint8_t*)m.data(), (uint32_t)m.size(), KLF_PAT_REGEX});
    klf_config cfg{};
    cfg.device = device;
    cfg.n_patterns = (uint32_t)pats.size();
    cfg.patterns = pats.empty() ? nullptr : pats.data();
    klf_engine* e = nullptr;
    int rc = klf_open(&cfg, &e);
    if (rc != KLF_OK) {
      std::string m = klf_strerror(rc);
      if (e) { m += std::string(": ") + klf_last_error(e); klf_close(e); }
      if (rc == KLF_EPATTERN || rc == KLF_ETOOBIG) {
        std::fprintf(stderr, "ERROR %s\n", m.c_str());
        return 1;
      }
      panic_exit(m);
    }
    if (klf_set_streams(e, n) != KLF_OK) panic_exit("klf_set_streams");
    std::vector<uint8_t> buf;
    for (uint32_t i = 0; i < n; ++i) {  // streamLog (:312-339): one body per stream
      if (body[i] == "-" || !read_file(body[i], buf)) {
        std::fprintf(stderr, "ERROR Error getting logs for container %s\n%s\n", cname[i].c_str(),
                     ("cannot read " + body[i]).c_str());
        continue;
      }
      if (!buf.empty() && klf_stage(e, i, buf.data(), buf.size()) != KLF_OK) panic_exit("klf_stage");
    }
    klf_result* r = nullptr;
    // context / inversion: the run itself with --tail 0 (the cheapest run that leaves the
    // line index and the match bitmap behind), then klf_regroup applies the user's tail
    const int64_t user_tail = filter.tail;
    if (regrouped || windowed || around || recorded) filter.tail = 0;
    rc = klf_run(e, &filter, &r);
    if (rc != KLF_OK) panic_exit(std::string("klf_run: ") + klf_strerror(rc) + ": " + klf_last_error(e));
    if (around) {  // (with the window, if any, in the one call)
      klf_result* g = nullptr;
      rc = klf_around(e, r, &around_opts, user_tail, &g);
      if (rc != KLF_OK) panic_exit(std::string("klf_around: ") + klf_strerror(rc) + ": " + klf_last_error(e));
      klf_result_free(r);
      r = g;
    } else if (recorded) {  // (with the window, if any, in the one call)
      klf_result* g = nullptr;
      rc = klf_records(e, r, &records_opts, user_tail, &g);
      if (rc != KLF_OK) panic_exit(std::string("klf_records: ") + klf_strerror(rc) + ": " + klf_last_error(e));
      klf_result_free(r);
      r = g;
    } else if (windowed) {  // (with the context flags, if any, in the one call)
      klf_result* g = nullptr;
      rc = klf_window(e, r, &window, user_tail, &g);
      if (rc != KLF_OK) panic_exit(std::string("klf_window: ") + klf_strerror(rc) + ": " + klf_last_error(e));
      klf_result_free(r);
      r = g;
    } else if (regrouped) {
      klf_result* g = nullptr;
      rc = klf_regroup(e, r, &regroup, user_tail, &g);
      if (rc != KLF_OK) panic_exit(std::string("klf_regroup: ") + klf_strerror(rc) + ": " + klf_last_error(e));
      klf_result_free(r);
      r = g;
    }
    if (hist_set) {  // over the result that gets written, before it is
      std::vector<uint64_t> hc((size_t)n * hist.n_buckets), ho((size_t)n * 2);
      rc = klf_result_histogram(r, &hist, hc.data(), ho.data(), nullptr);
      if (rc != KLF_OK) panic_exit(std::string("klf_result_histogram: ") + klf_strerror(rc) + ": " + klf_last_error(e));
      const std::string hpath = logpath + "/histogram.tsv";
      FILE* hf = std::fopen(hpath.c_str(), "w");
      if (!hf) panic_exit("create " + hpath);
      std::fprintf(hf, "Pod\tContainer\tBucket\tLines\n");
      for (uint32_t i = 0; i < n; ++i) {
        const char* pod = pods[table[i].pod].name.c_str();
        if (ho[2 * (size_t)i])
          std::fprintf(hf, "%s\t%s\tbelow\t%llu\n", pod, cname[i].c_str(), (unsigned long long)ho[2 * (size_t)i]);
        for (uint32_t k = 0; k < hist.n_buckets; ++k) {
          const uint64_t c = hc[(size_t)i * hist.n_buckets + k];
          if (!c) continue;
          const __int128 t = (__int128)hist.origin.sec * 1000000000 + hist.origin.nsec + (__int128)k * hist.width_ns;
          __int128 sec = t / 1000000000, ns = t % 1000000000;
          if (ns < 0) { ns += 1000000000; --sec; }
          const time_t ts = (time_t)sec;
          struct tm tm;
          gmtime_r(&ts, &tm);
          std::fprintf(hf, "%s\t%s\t%04d-%02d-%02dT%02d:%02d:%02d.%09dZ\t%llu\n", pod, cname[i].c_str(),
                       tm.tm_year + 1900, tm.tm_mon + 1, tm.tm_mday, tm.tm_hour, tm.tm_min, tm.tm_sec, (int)ns,
                       (unsigned long long)c);
        }
        if (ho[2 * (size_t)i + 1])
          std::fprintf(hf, "%s\t%s\tabove\t%llu\n", pod, cname[i].c_str(), (unsigned long long)ho[2 * (size_t)i + 1]);
      }
      if (std::fclose(hf) != 0) panic_exit("close " + hpath);
    }
    if (top_set) {  // the most frequent messages of the result that gets written, before it is
      klf_groups* gr = nullptr;
      rc = klf_result_groups(r, &top, &gr);
      if (rc != KLF_OK) panic_exit(std::string("klf_result_groups: ") + klf_strerror(rc) + ": " + klf_last_error(e));
      const klf_group_entry* ge = nullptr;
      const uint8_t* keys = nullptr;
      uint64_t ng = 0, nk = 0;
      rc = klf_groups_entries(gr, &ge, &ng);
      if (rc == KLF_OK) rc = klf_groups_keys(gr, &keys, &nk);
      if (rc != KLF_OK) panic_exit(std::string("klf_groups_entries: ") + klf_strerror(rc) + ": " + klf_last_error(e));
      const std::string tpath = logpath + "/top.tsv";
      FILE* tf = std::fopen(tpath.c_str(), "w");
      if (!tf) panic_exit("create " + tpath);
      std::fprintf(tf, "Lines\tFirstPod\tFirstContainer\tFirstLine\tLastPod\tLastContainer\tLastLine\tKey\n");
      for (uint64_t k = 0; k < ng; ++k) {
        const klf_group_entry& x = ge[k];
        std::fprintf(tf, "%llu\t%s\t%s\t%llu\t%s\t%s\t%llu\t", (unsigned long long)x.count,
                     pods[table[x.first_stream].pod].name.c_str(), cname[x.first_stream].c_str(),
                     (unsigned long long)x.first_line + 1, pods[table[x.last_stream].pod].name.c_str(),
                     cname[x.last_stream].c_str(), (unsigned long long)x.last_line + 1);
        for (uint32_t b = 0; b < x.key_len; ++b) {  // every byte outside printable ASCII, and '\\', as \xHH
          const uint8_t c = keys[x.key_off + b];
          if (c < 0x20 || c >= 0x7f || c == '\\') std::fprintf(tf, "\\x%02X", c);
          else std::fputc(c, tf);
        }
        std::fputc('\n', tf);
      }
      if (std::fclose(tf) != 0) panic_exit("close " + tpath);
      klf_groups_free(gr);
    }
    if (stat_set) {  // the field's statistics over the result that gets written, before it is
      static const uint16_t quantiles[3] = {5000, 9000, 9900};  // p50, p90, p99
      const klf_field_opts fo{(const uint8_t*)stat_key.data(), quantiles, (uint32_t)stat_key.size(), stat_decimals, 3,
                              stat_duration ? KLF_FIELD_DURATION : 0u};
      std::vector<klf_field_row> fr((size_t)n + 1);
      std::vector<int64_t> fq(((size_t)n + 1) * 3);
      rc = klf_result_field_stats(r, &fo, fr.data(), fq.data(), nullptr);
      if (rc != KLF_OK) panic_exit(std::string("klf_result_field_stats: ") + klf_strerror(rc) + ": " + klf_last_error(e));
      const std::string spath = logpath + "/stats.tsv";
      FILE* sf = std::fopen(spath.c_str(), "w");
      if (!sf) panic_exit("create " + spath);
      auto fixed = [&](__int128 v) {  // a fixed-point value with stat_decimals fraction digits
        if (v < 0) { std::fputc('-', sf); v = -v; }
        __int128 scale = 1;
        for (uint32_t k = 0; k < stat_decimals; ++k) scale *= 10;
        char buf[48];
        int len = 0;
        __int128 ip = v / scale;
        do { buf[len++] = (char)('0' + (int)(ip % 10)); ip /= 10; } while (ip);
        while (len) std::fputc(buf[--len], sf);
        if (stat_decimals) std::fprintf(sf, ".%0*llu", (int)stat_decimals, (unsigned long long)(v % scale));
      };
      for (uint32_t i = 0; i <= n; ++i) {
        const klf_field_row& x = fr[i];
        std::fprintf(sf, "%s\t%s\t%llu\t%llu\t%llu", i < n ? pods[table[i].pod].name.c_str() : "*",
                     i < n ? cname[i].c_str() : "*", (unsigned long long)x.lines, (unsigned long long)x.hits,
                     (unsigned long long)x.bad);
        if (!x.hits || x.max_stream >= n) {
          std::fprintf(sf, "\t-\t-\t-\t-\t-\t-\t-\n");
          continue;
        }
        const __int128 sum = (__int128)x.sum_hi * ((__int128)1 << 64) + (__int128)x.sum_lo;
        for (const __int128 v : {(__int128)x.min, (__int128)x.max, sum, (__int128)fq[3 * (size_t)i],
                                 (__int128)fq[3 * (size_t)i + 1], (__int128)fq[3 * (size_t)i + 2]}) {
          std::fputc('\t', sf);
          fixed(v);
        }
        std::fprintf(sf, "\t%s/%s:%llu\n", pods[table[x.max_stream].pod].name.c_str(), cname[x.max_stream].c_str(),
                     (unsigned long long)x.max_line + 1);
      }
      if (std::fclose(sf) != 0) panic_exit("close " + spath);
    }
    if (merge) {  // the timeline of the result that gets written, beside the per-container files
      std::string tags;
      std::vector<uint32_t> tag_off(n + 1, 0);
      for (uint32_t i = 0; i < n; ++i) {
        std::string tag = pods[table[i].pod].name + "/" + cname[i];
        if (tag.size() > KLF_TIMELINE_MAX_TAG - 1) tag.resize(KLF_TIMELINE_MAX_TAG - 1);
        tags += tag + " ";
        tag_off[i + 1] = (uint32_t)tags.size();
      }
      const klf_timeline_opts topts{(const uint8_t*)tags.data(), tag_off.data(), merge_ts ? KLF_TIMELINE_TIMESTAMPS : 0u, 0};
      klf_timeline* tl = nullptr;
      rc = klf_result_timeline(r, &topts, &tl);
      if (rc != KLF_OK) panic_exit(std::string("klf_result_timeline: ") + klf_strerror(rc) + ": " + klf_last_error(e));
      const std::string mpath = logpath + "/merged.log";
      const int mfd = ::open(mpath.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
      if (mfd < 0) panic_exit("create " + mpath);
      rc = klf_timeline_write(tl, mfd, nullptr);
      if (rc != KLF_OK) panic_exit(std::string("klf_timeline_write: ") + klf_strerror(rc) + ": " + klf_last_error(e));
      if (::close(mfd) != 0) panic_exit("close " + mpath);
      klf_timeline_free(tl);
    }
    // writeLogToDisk (:359-374): one klf_result_write over every stream's file (chunked,
    // double-buffered D2H from pinned memory), files closed afterwards
    std::vector<int> fds(n, -1);
    for (uint32_t i = 0; i < n; ++i) {
      fds[i] = ::open(files[i].c_str(), O_WRONLY | O_TRUNC);
      if (fds[i] < 0) panic_exit("open " + files[i]);
    }
    rc = klf_result_write(r, fds.data(), n, nullptr);
    if (rc != KLF_OK) panic_exit(std::string("klf_result_write: ") + klf_strerror(rc) + ": " + klf_last_error(e));
    for (uint32_t i = 0; i < n; ++i)
      if (::close(fds[i]) != 0) panic_exit("close " + files[i]);
    klf_result_free(r);
    klf_close(e);
  }

  // printLogSize (:279-309)
  if (n == 0) {
    std::fprintf(stdout, "ERROR No logs saved\n");
    return 0;
  }
  std::fprintf(stdout, "INFO  Logs saved to %s\n", logpath.c_str());
  std::fprintf(stdout, "Pod\tContainer\tSize\n");
  for (uint32_t i = 0; i < n; ++i) {
    struct stat st;
    if (stat(files[i].c_str(), &st) != 0) continue;
    char sz[64];
    klh_convert_bytes((int64_t)st.st_size, color ? 1 : 0, sz, sizeof(sz));
    std::fprintf(stdout, "%s\t%s\t%s\n", pods[table[i].pod].name.c_str(), cname[i].c_str(), sz);
  }
  return 0;
}
