// Stand-alone check of rtlsdrdiags_amd/csrc/iqd_tool.h - the part of the command-line tools that needs no library - built with
// AddressSanitizer and UBSan by tests/test_tool_args.py.  argv[1]: a directory to write the number files into.
#include <math.h>

#include "iqd_tool.h"

using namespace iqdtool;

#define CHECK(x)                                             \
  do {                                                       \
    if (!(x)) {                                              \
      printf("%s:%d: %s\n", __FILE__, __LINE__, #x);        \
      return 1;                                              \
    }                                                        \
  } while (0)

static bool run(const std::vector<Row> &rows, std::vector<const char *> args, const char *tool = nullptr)
{
  args.insert(args.begin(), "tool");
  return parse((int)args.size(), const_cast<char **>(args.data()), rows, tool);
}

// rows as iqdemod_wide declares them: every conversion, the P[/Q] row, the whole word before its prefix, the band keys
struct Wide {
  std::string in, format = "u8";
  double rate = 0;
  uint32_t blocks = 4, m = 0, den = 1, tracks = 0;
  int rotation = 1;
  uint64_t centre = 0;
  bool mGiven = false, autoModes = false;
  std::vector<double> modes;
  std::vector<std::string> agc;
  BandArgs band;
  std::vector<Row> keys()
  {
    std::vector<Row> t = {text("in=", in), text("format=", format), real("rate=", rate), viaAtoi("blocks=", blocks), viaAtoi("rotation=", rotation),
                          viaStrtoull("centre=", centre), u32("tracks=", tracks),
                          {"decimation=", [this](const char *v) {
                             const char *slash = strchr(v, '/');
                             m = (uint32_t)atoi(v);
                             den = slash ? (uint32_t)atoi(slash + 1) : 1;
                             return true;
                           }, &mGiven},
                          word("modes=auto", [this] { autoModes = true; modes = {2.0}; }),
                          {"modes=", [this](const char *v) { modes = doubleList(v); return true; }},
                          {"agc=", [this](const char *v) { agc = nameList(v); return true; }}};
    band.rows(t, "check");
    return t;
  }
};

static int checkTable()
{
  {
    Wide w;   // a repeated key: the last wins; each conversion as the tools have it
    CHECK(run(w.keys(), {"in=a", "rate=1e3", "rate=2400000.5", "blocks=0x10", "rotation=-1", "centre=100000000000", "tracks=0x4", "decimation=75/8",
                         "in=b", "format=s8", "bias=0x10", "rank=0x10", "margin=7", "edges=2,4,8", "maxdet=4junk"}));
    CHECK(w.in == "b" && w.format == "s8" && w.rate == 2400000.5 && w.blocks == 0 && w.rotation == -1 && w.centre == 100000000000ull);
    CHECK(w.tracks == 0 && w.m == 75 && w.den == 8 && w.mGiven && !w.autoModes);
    CHECK(w.band.tc.inc_bias == 16 && w.band.dc.floor_rank == 0 && w.band.rankGiven && w.band.mc.margin == 7 && w.band.marginGiven);
    CHECK(w.band.edgesGiven && w.band.tc.class_edge[0] == 2 && w.band.tc.class_edge[1] == 4 && w.band.tc.class_edge[2] == 8);
    CHECK(w.band.dc.max_detections == 4 && !w.band.wideGiven);
  }
  {
    Wide w;   // the whole word before its prefix, both ways round, and a word that only starts like it
    CHECK(run(w.keys(), {"modes=auto"}) && w.autoModes && w.modes == std::vector<double>{2.0});
    CHECK(run(w.keys(), {"modes=1,3"}) && w.autoModes && (w.modes == std::vector<double>{1.0, 3.0}));
    Wide x;
    CHECK(run(x.keys(), {"modes=autox", "decimation=8"}) && !x.autoModes && x.modes == std::vector<double>{0.0} && x.m == 8 && x.den == 1);
  }
  for (int at = 0; at < 3; at++) {   // an unknown key first, in the middle, last: nothing behind it is read
    Wide w;
    std::vector<const char *> args = {"in=a", "blocks=2"};
    args.insert(args.begin() + at, "block=9");
    CHECK(!run(w.keys(), args, "check"));
    CHECK(w.in == (at >= 1 ? "a" : "") && w.blocks == (at == 2 ? 2u : 4u));
  }
  {
    Wide w;   // edges= refuses by itself, at once
    CHECK(!run(w.keys(), {"edges=1,2", "in=a"}) && !w.band.edgesGiven && w.in.empty());
    CHECK(!run(w.keys(), {"in"}) && !run(w.keys(), {""}) && !run(w.keys(), {"IN=a"}));
    CHECK(run(w.keys(), {}) && run(w.keys(), {"in="}) && w.in.empty());
  }
  {
    // iqdemod_spectrum: the band keys, slots= and the track log's; strtoul base 10 but for bias=
    BandArgs b;
    std::string out;
    uint32_t bins = 0;
    std::vector<Row> t = {text("out=", out), u32("bins=", bins)};
    b.rows(t, "check");
    b.logRows(t);
    CHECK(run(t, {"bins=0x40", "bins=128x", "slots=3", "minactive=5", "votemin=6", "maxevents=7", "rank=9", "ratio_q8=10", "guard=2", "bridge=3", "minwidth=4",
                  "maxdet=5", "gate_q8=11", "open=12", "hold=13", "alpha_q8=14", "bias=010", "margin=1", "beta_q16=15", "carrier=2", "minsum=16",
                  "carrier_q8=17", "wide=18", "out=x=y"}));
    CHECK(bins == 128 && out == "x=y" && b.tc.n_slots == 3 && b.lc.min_active == 5 && b.lc.vote_min == 6 && b.lc.max_events == 7);
    CHECK(b.dc.floor_rank == 9 && b.dc.ratio_q8 == 10 && b.dc.dc_guard == 2 && b.dc.bridge == 3 && b.dc.min_width == 4 && b.dc.max_detections == 5);
    CHECK(b.tc.gate_q8 == 11 && b.tc.open_hits == 12 && b.tc.hold_blocks == 13 && b.tc.alpha_q8 == 14 && b.tc.inc_bias == 8);
    CHECK(b.mc.margin == 1 && b.mc.obw_tail_q16 == 15 && b.mc.carrier_half == 2 && b.mc.min_sum == 16 && b.mc.carrier_min_q8 == 17 && b.mc.wide_bins == 18);
    CHECK(b.rankGiven && b.marginGiven && b.wideGiven && !b.edgesGiven);
  }
  {
    // iqdemod_filter: chunk= through strtoull; iqdemod_multi: atoi, two whole words, no message of parse's own
    size_t chunk = 65536;
    uint32_t factor = 1;
    CHECK(run({u32("factor=", factor), viaStrtoull("chunk=", chunk)}, {"chunk=4294967296", "factor=-1"}) && chunk == 4294967296ull && factor == 0xffffffffu);
    uint32_t channels = 0;
    int threshold = -200, agc = -1;
    bool interleaved = false;
    std::vector<int> modes{2};
    const std::vector<Row> t = {viaAtoi("channels=", channels), viaAtoi("threshold=", threshold), viaAtoi("agc=", agc),
                                {"modes=", [&modes](const char *v) { modes = intList(v); return true; }},
                                word("layout=files", [&] { interleaved = false; }), word("layout=interleaved", [&] { interleaved = true; })};
    CHECK(run(t, {"channels=0x2", "threshold=-60dB", "agc=1", "modes=2,3,", "layout=interleaved"}));
    CHECK(channels == 0 && threshold == -60 && agc == 1 && (modes == std::vector<int>{2, 3}) && interleaved);
    CHECK(run(t, {"layout=files", "modes="}) && !interleaved && modes.empty());
    CHECK(!run(t, {"layout=file"}) && !run(t, {"layout=filesx"}) && !run(t, {"layout="}));
  }
  return 0;
}

static int checkLists()
{
  CHECK(doubleList("").empty() && intList("").empty() && u64List("").empty());
  CHECK(doubleList("1") == std::vector<double>{1.0} && doubleList("1,") == std::vector<double>{1.0});
  CHECK((doubleList(",1") == std::vector<double>{0.0, 1.0}) && (doubleList("a,2") == std::vector<double>{0.0, 2.0}));
  CHECK((intList("a,2") == std::vector<int>{0, 2}) && (intList("-1,0,1") == std::vector<int>{-1, 0, 1}) && intList(",") == std::vector<int>{0});
  CHECK((u64List("100000000000,2,") == std::vector<uint64_t>{100000000000ull, 2}) && (u64List(",1") == std::vector<uint64_t>{0, 1}));
  // agc='s names keep their empty items, so that the tool can refuse them
  CHECK(nameList("") == std::vector<std::string>{""} && nameList("1") == std::vector<std::string>{"1"});
  CHECK((nameList("1,") == std::vector<std::string>{"1", ""}) && (nameList(",1") == std::vector<std::string>{"", "1"}));
  CHECK((nameList("a,2") == std::vector<std::string>{"a", "2"}) && (nameList("harris,off,lowpass") == std::vector<std::string>{"harris", "off", "lowpass"}));
  return 0;
}

static bool put(const std::string &path, const char *text)
{
  FILE *f = fopen(path.c_str(), "w");
  return f && fputs(text, f) >= 0 && fclose(f) == 0;
}

static int checkNumbers(const std::string &dir)
{
  const auto int16 = [](const char *tok, int16_t &x) {
    char *end = nullptr;
    const long v = strtol(tok, &end, 10);
    x = (int16_t)v;
    return *end == 0 && v >= -32768 && v <= 32767;
  };
  const auto real = [](const char *tok, float &x) {
    x = strtof(tok, nullptr);
    return true;
  };
  const std::string p = dir + "/numbers.txt";
  std::vector<int16_t> w;
  CHECK(put(p, "1, 2,3\n-4 \t5,6,\r\n 7\n32767 -32768") && readNumbers(p, w, int16));
  CHECK((w == std::vector<int16_t>{1, 2, 3, -4, 5, 6, 7, 32767, -32768}));
  w.clear();   // a comma belongs straight behind its number: one that stands alone ends the reading there, as it always has
  CHECK(put(p, "1,2 ,3") && readNumbers(p, w, int16) && (w == std::vector<int16_t>{1, 2}));
  for (const char *bad : {"1 40000 2", "1 -32769", "1 2x", "1 99999999999999999999 2", "1.5"}) {   // out of range, or no number: all tokens are kept
    w.clear();
    CHECK(put(p, bad) && !readNumbers(p, w, int16) && !w.empty());
  }
  for (const char *none : {"", " ,\n, \n", "\n"}) {
    w.clear();
    CHECK(put(p, none) && !readNumbers(p, w, int16) && w.empty());
  }
  CHECK(!readNumbers(dir + "/none.txt", w, int16));
  std::vector<float> h;
  CHECK(put(p, "0.5,-0.25\n1e-3 junk,\n") && readNumbers(p, h, real) && (h == std::vector<float>{0.5f, -0.25f, 1e-3f, 0.0f}));
  const std::string longToken(300, '7');   // cut into tokens of 127 characters: no overrun
  w.clear();
  CHECK(put(p, longToken.c_str()) && !readNumbers(p, w, int16) && w.size() == 3);
  return 0;
}

static int checkNamesAndFiles(const std::string &dir)
{
  CHECK(channelName("pcm_%d.s16", 7) == "pcm_7.s16" && channelName("plain", 3) == "plain");
  const std::string a(3998, 'a');
  CHECK(channelName(a + "%d", 123456) == a + "123456");                  // 4004 characters fit
  CHECK(channelName(std::string(5000, 'b') + "%d", 1) == std::string(4095, 'b'));   // cut at the buffer, terminated
  Files files("check");
  FILE *out = files.open(dir + "/out.bin", "wb", Files::Quiet);
  CHECK(out && fputs("xyz", out) >= 0);
  CHECK(!files.open(dir + "/none/out.bin", "wb", Files::Named) && !files.open(dir + "/none.bin", "rb", Files::Perror));
  CHECK(files.close() && files.close());                                 // (twice: nothing is closed twice)
  FILE *in = files.open(dir + "/out.bin", "rb", Files::Named);
  char buf[8] = {0};
  CHECK(in && fread(buf, 1, 8, in) == 3 && !strcmp(buf, "xyz"));
  return 0;   // (the destructor closes `in`: the leak check sees it if not)
}

// derive() against the formulas of the tools' usage comments
static int checkDerive()
{
  for (uint32_t N : {64u, 128u, 256u, 512u, 1024u, 2048u})
    for (int given = 0; given < 16; given++) {
      BandArgs b;
      std::vector<Row> t;
      b.rows(t, "check");
      std::vector<const char *> args = {"guard=3", "maxdet=5"};
      if (given & 1) args.push_back("rank=7");
      if (given & 2) args.push_back("edges=1,2,3");
      if (given & 4) args.push_back("margin=0");
      if (given & 8) args.push_back("wide=9");
      CHECK(run(t, args));
      const uint32_t S = 1 + given;
      b.derive(N, S);
      CHECK(b.dc.n_bins == N && b.tc.n_bins == N && b.mc.n_bins == N && b.tc.n_slots == S && b.mc.n_slots == S && b.lc.n_slots == S);
      CHECK(b.tc.n_sources == 1 && b.mc.n_sources == 1 && b.lc.n_sources == 1);
      CHECK(b.tc.max_detections == 5 && b.mc.dc_guard == 3 && b.dc.dc_guard == 3);
      CHECK(b.dc.floor_rank == (given & 1 ? 7 : N / 2));
      const uint32_t e0 = given & 2 ? 1 : N / 64 + 1, e1 = given & 2 ? 2 : N / 16, e2 = given & 2 ? 3 : N / 4;
      CHECK(b.tc.class_edge[0] == e0 && b.tc.class_edge[1] == e1 && b.tc.class_edge[2] == e2);
      CHECK(b.mc.margin == (given & 4 ? 0 : N < 256 ? 1 : N / 256) && b.mc.wide_bins == (given & 8 ? 9 : N / 32));
      // what no key touched is the default of the usage comments
      CHECK(b.dc.ratio_q8 == 2048 && b.dc.bridge == 8 && b.dc.min_width == 3 && b.tc.gate_q8 == 512 && b.tc.open_hits == 3 && b.tc.hold_blocks == 2);
      CHECK(b.tc.alpha_q8 == 64 && b.tc.inc_bias == 0 && b.mc.obw_tail_q16 == 328 && b.mc.carrier_half == 1 && b.mc.min_sum == 4096);
      CHECK(b.mc.carrier_min_q8 == 160 && b.lc.max_events == 256 && b.lc.min_active == 2 && b.lc.vote_min == 4);
    }
  BandArgs b;
  CHECK(b.tc.n_slots == 8 && b.dc.max_detections == 16 && b.dc.dc_guard == 1);
  return 0;
}

int main(int argc, char **argv)
{
  if (argc != 2) return 2;
  if (checkTable() || checkLists() || checkNumbers(argv[1]) || checkNamesAndFiles(argv[1]) || checkDerive()) return 1;
  printf("tool args ok\n");
  return 0;
}
