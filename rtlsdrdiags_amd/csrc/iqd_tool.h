// iqd_tool.h — what the command-line tools (iqdemod_wide, _spectrum, _filter, _multi) share and what can be checked without
// the library: it includes include/iqdemod.h for the config structs and calls no iqd_* function
// (tests/tool_args/tool_args_check.cpp runs all of it under AddressSanitizer and UBSan).
//   Row, parse()      a tool's key= arguments as one table: a new key is one row
//   splitList()       "a,b,c" with one conversion per element
//   readNumbers()     a text file of numbers separated by white space or commas
//   channelName()     out=pcm_%d.s16 and its like
//   Files             the files a tool opened, closed on every way out
//   BandArgs          the band chain's configs: defaults, rows, and derive() for every value that was left out
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <functional>
#include <string>
#include <vector>

#include "iqdemod.h"

namespace iqdtool {

// ---- the key= table ----------------------------------------------------------------------------------------------------------
// A key that ends in '=' matches as a prefix and hands the rest to `set`; any other key is a whole word (modes=auto).  Rows
// are tried in order, so a whole word stands before the prefix it would also match.  set() returning false ends the parse: it
// has printed its own message.
struct Row {
  const char *key;
  std::function<bool(const char *)> set;
  bool *given = nullptr;
};

inline Row text(const char *key, std::string &d) { return {key, [&d](const char *v) { d = v; return true; }}; }
inline Row real(const char *key, double &d) { return {key, [&d](const char *v) { d = atof(v); return true; }}; }
template <class T> Row viaAtoi(const char *key, T &d) { return {key, [&d](const char *v) { d = (T)atoi(v); return true; }}; }
template <class T> Row viaStrtoull(const char *key, T &d) { return {key, [&d](const char *v) { d = (T)strtoull(v, nullptr, 10); return true; }}; }
inline Row u32(const char *key, uint32_t &d, bool *given = nullptr, int base = 10)
{
  return {key, [&d, base](const char *v) { d = (uint32_t)strtoul(v, nullptr, base); return true; }, given};
}
inline Row word(const char *key, std::function<void()> f) { return {key, [f](const char *) { f(); return true; }}; }

// tool: the name in "<tool>: unknown argument %s"; nullptr: the caller prints its own usage
inline bool parse(int argc, char **argv, const std::vector<Row> &rows, const char *tool)
{
  for (int i = 1; i < argc; i++) {
    const char *a = argv[i];
    const Row *hit = nullptr;
    for (const Row &r : rows) {
      const size_t n = strlen(r.key);
      if (n && r.key[n - 1] == '=' ? !strncmp(a, r.key, n) : !strcmp(a, r.key)) {
        hit = &r;
        break;
      }
    }
    if (!hit) {
      if (tool) fprintf(stderr, "%s: unknown argument %s\n", tool, a);
      return false;
    }
    if (!hit->set(a + strlen(hit->key))) return false;
    if (hit->given) *hit->given = true;
  }
  return true;
}

// ---- lists -------------------------------------------------------------------------------------------------------------------
// conv(first, end) makes one element of [first, end), end == nullptr: up to the string's end (atof and its kin stop at the
// comma by themselves).  An empty string gives an empty list and a trailing comma adds nothing - unless emptyItems: then ""
// is one empty element and "a," two (agc=, whose names are then refused).
template <class T, class F> std::vector<T> splitList(const char *s, F conv, bool emptyItems = false)
{
  std::vector<T> v;
  for (const char *q = s; emptyItems || *q;) {
    const char *c = strchr(q, ',');
    v.push_back(conv(q, c));
    if (!c) break;
    q = c + 1;
  }
  return v;
}
inline std::vector<double> doubleList(const char *s) { return splitList<double>(s, [](const char *q, const char *) { return atof(q); }); }
inline std::vector<int> intList(const char *s) { return splitList<int>(s, [](const char *q, const char *) { return atoi(q); }); }
inline std::vector<uint64_t> u64List(const char *s)
{
  return splitList<uint64_t>(s, [](const char *q, const char *) { return (uint64_t)strtoull(q, nullptr, 10); });
}
inline std::vector<std::string> nameList(const char *s)
{
  return splitList<std::string>(s, [](const char *q, const char *c) { return c ? std::string(q, c) : std::string(q); }, true);
}

// ---- number files --------------------------------------------------------------------------------------------------------------
// conv(token, value) -> false: not a number of this file's kind.  True if every token was one and there was at least one.
template <class T, class F> bool readNumbers(const std::string &path, std::vector<T> &v, F conv)
{
  FILE *f = fopen(path.c_str(), "r");
  if (!f) return false;
  char tok[128];
  bool ok = true;
  while (fscanf(f, " %127[^ \t\r\n,]", tok) == 1) {
    T x{};
    if (!conv(tok, x)) ok = false;
    v.push_back(x);
    int c = fgetc(f);
    if (c != ',' && c != EOF) ungetc(c, f);
  }
  fclose(f);
  return ok && !v.empty();
}

inline std::string channelName(const std::string &pattern, uint32_t c)
{
  char name[4096];
  snprintf(name, sizeof(name), pattern.c_str(), (int)c);
  return name;
}

// ---- files ---------------------------------------------------------------------------------------------------------------------
class Files {
 public:
  enum Say { Quiet, Named, Perror };   // a failed open: nothing / "<tool>: cannot open|create %s" / perror(path)
  explicit Files(const char *tool) : tool_(tool) {}
  Files(const Files &) = delete;
  Files &operator=(const Files &) = delete;
  ~Files() { close(); }
  FILE *open(const std::string &path, const char *mode, Say say)
  {
    FILE *f = fopen(path.c_str(), mode);
    if (f) open_.push_back({f, mode[0] != 'r'});
    else if (say == Named) fprintf(stderr, "%s: cannot %s %s\n", tool_, mode[0] == 'r' ? "open" : "create", path.c_str());
    else if (say == Perror) perror(path.c_str());
    return f;
  }
  // false: an output did not close cleanly (spectrum and filter make that status 1; the destructor does not look)
  bool close()
  {
    bool ok = true;
    for (const Open &o : open_)
      if (fclose(o.f) != 0 && o.output) ok = false;
    open_.clear();
    return ok;
  }

 private:
  struct Open {
    FILE *f;
    bool output;
  };
  const char *tool_;
  std::vector<Open> open_;
};

// ---- the band chain's arguments ------------------------------------------------------------------------------------------------
struct BandArgs {
  iqd_detect_config dc{};
  iqd_track_config tc{};
  iqd_measure_config mc{};
  iqd_tracklog_config lc{};
  bool rankGiven = false, edgesGiven = false, marginGiven = false, wideGiven = false;
  BandArgs()
  {
    dc.ratio_q8 = 2048;
    dc.dc_guard = 1;
    dc.bridge = 8;
    dc.min_width = 3;
    dc.max_detections = 16;
    tc.n_sources = mc.n_sources = lc.n_sources = 1;
    tc.n_slots = 8;
    tc.gate_q8 = 512;
    tc.open_hits = 3;
    tc.hold_blocks = 2;
    tc.alpha_q8 = 64;
    mc.obw_tail_q16 = 328;
    mc.carrier_half = 1;
    mc.min_sum = 4096;
    mc.carrier_min_q8 = 160;
    lc.max_events = 256;
    lc.min_active = 2;
    lc.vote_min = 4;
  }
  // the detector's, the tracker's and the measurements' keys, the same in every tool
  void rows(std::vector<Row> &t, const char *tool)
  {
    t.insert(t.end(), {u32("rank=", dc.floor_rank, &rankGiven), u32("ratio_q8=", dc.ratio_q8), u32("guard=", dc.dc_guard), u32("bridge=", dc.bridge),
                       u32("minwidth=", dc.min_width), u32("maxdet=", dc.max_detections), u32("gate_q8=", tc.gate_q8), u32("open=", tc.open_hits),
                       u32("hold=", tc.hold_blocks), u32("alpha_q8=", tc.alpha_q8), u32("bias=", tc.inc_bias, nullptr, 0),
                       u32("margin=", mc.margin, &marginGiven), u32("beta_q16=", mc.obw_tail_q16), u32("carrier=", mc.carrier_half),
                       u32("minsum=", mc.min_sum), u32("carrier_q8=", mc.carrier_min_q8), u32("wide=", mc.wide_bins, &wideGiven)});
    t.push_back({"edges=", [this, tool](const char *v) {
                   edgesGiven = sscanf(v, "%u,%u,%u", &tc.class_edge[0], &tc.class_edge[1], &tc.class_edge[2]) == 3;
                   if (!edgesGiven) fprintf(stderr, "%s: edges= takes three widths in bins, a,b,c\n", tool);
                   return edgesGiven;
                 }});
  }
  // the track log's keys, and the slot count where no channel count stands for it
  void logRows(std::vector<Row> &t)
  {
    t.insert(t.end(), {u32("slots=", tc.n_slots), u32("minactive=", lc.min_active), u32("votemin=", lc.vote_min), u32("maxevents=", lc.max_events)});
  }
  // every value the user left out or cannot give: the sizes, what one object carries over from another, the defaults in bins
  void derive(uint32_t bins, uint32_t slots)
  {
    dc.n_bins = tc.n_bins = mc.n_bins = bins;
    tc.n_slots = mc.n_slots = lc.n_slots = slots;
    tc.max_detections = dc.max_detections;
    mc.dc_guard = dc.dc_guard;
    if (!rankGiven) dc.floor_rank = bins / 2;
    if (!edgesGiven) {
      tc.class_edge[0] = bins / 64 + 1;
      tc.class_edge[1] = bins / 16;
      tc.class_edge[2] = bins / 4;
    }
    if (!marginGiven) mc.margin = bins / 256 ? bins / 256 : 1;
    if (!wideGiven) mc.wide_bins = bins / 32;
  }
};

}  // namespace iqdtool
