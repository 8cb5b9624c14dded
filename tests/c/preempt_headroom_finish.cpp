/* preempt_headroom_finish.cpp — the finish step of ykpred_preempt_headroom (csrc/engine/preempt_headroom_finish.h: per-level deltas → the
 * 32 cells of one ask) and the argument errors of the ykhost_preempt_headroom* calls on a MIRROR-ONLY handle (device -1), for a build
 * under AddressSanitizer + UBSan together with libykhost's sources (tests/test_preempt_headroom_cpu.py). No device is touched.
 *
 *   preempt_headroom_finish <cases file>
 * Every line of the file is one case: limit want coupled d[0] ... d[31]; the program prints the 32 cells of each, one line per case,
 * then runs the host checks. Exit code 0 and a last line "preempt headroom ok" = every call behaved. */
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../yunikorn-k8shim_amd/csrc/engine/preempt_headroom_finish.h"
#include "ykhost.h"
#include "ykpred.h"

static int failures = 0;
#define EXPECT(cond)                                                \
  do {                                                              \
    if (!(cond)) {                                                  \
      fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); \
      failures++;                                                   \
    }                                                               \
  } while (0)

static const char* kSnapshot =
    "{\"nodes\":[{\"metadata\":{\"name\":\"n0\"},\"status\":{\"allocatable\":{\"cpu\":\"4\",\"memory\":\"1000\",\"pods\":\"10\"}},\"pods\":["
    "{\"metadata\":{\"name\":\"a\",\"uid\":\"a\",\"namespace\":\"d\"},\"spec\":{\"priority\":5,\"containers\":[{\"name\":\"c\",\"resources\":{\"requests\":{\"cpu\":\"100m\"}}}]}}]}],"
    "\"pods\":[{\"metadata\":{\"name\":\"ask\",\"uid\":\"ask\",\"namespace\":\"d\"},\"spec\":{\"priority\":9,\"containers\":[{\"name\":\"c\","
    "\"resources\":{\"requests\":{\"cpu\":\"50m\"}}}]}}]}";

int main(int argc, char** argv) {
  static_assert(ykfinish::kPreemptHeadroomCells == YKPRED_PREEMPT_HEADROOM_CELLS, "the finish writes the layout of ykpred.h");
  if (argc < 2) {
    fprintf(stderr, "usage: %s <cases file>\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  for (;;) {
    long long limit = 0, want = 0, coupled = 0;
    if (fscanf(f, "%lld %lld %lld", &limit, &want, &coupled) != 3) break;
    std::vector<int64_t> deltas(YKPRED_PREEMPT_HEADROOM_CELLS), out(YKPRED_PREEMPT_HEADROOM_CELLS, 0x5555);  // (exactly 32: a write past the row is caught)
    for (auto& d : deltas) {
      long long v = 0;
      if (fscanf(f, "%lld", &v) != 1) return 2;
      d = v;
    }
    ykfinish::preempt_headroom_finish(deltas.data(), limit, want, coupled != 0, out.data());
    for (size_t c = 0; c < out.size(); ++c) printf("%" PRId64 "%c", out[c], c + 1 == out.size() ? '\n' : ' ');
  }
  fclose(f);

  /* the host calls on a handle without a device: argument errors first, then "no device", with the cells as promised */
  char err[256] = "";
  ykhost_t* h = ykhost_create(-1, err, sizeof err);
  if (!h) {
    fprintf(stderr, "ykhost_create(-1): %s\n", err);
    return 2;
  }
  EXPECT(ykhost_load_snapshot(h, kSnapshot) == 0);
  int64_t cells[YKPRED_PREEMPT_HEADROOM_CELLS];
  int32_t rows[9], limit = -7;
  const int32_t ask0 = 0, bounds[2] = {1, 8};
  const int64_t zero = 0, two = 2;
  EXPECT(ykhost_preempt_headroom(h, -1, NULL, NULL, cells) == -1);
  EXPECT(ykhost_preempt_headroom(h, 1, &ask0, NULL, NULL) == -1);
  EXPECT(ykhost_preempt_headroom(h, 1, &ask0, &zero, cells) == YKPRED_E_INVALID);   /* a want below 1, before anything else */
  EXPECT(ykhost_preempt_headroom(h, 1, &ask0, &two, cells) == YKPRED_E_STATE);      /* no device */
  EXPECT(ykhost_preempt_headroom_nodes(h, 0, NULL, &limit) == -1);
  EXPECT(ykhost_preempt_headroom_nodes(h, 0, rows, NULL) == -1);
  EXPECT(ykhost_preempt_headroom_nodes(h, 0, rows, &limit) == YKPRED_E_STATE && limit == -7);
  EXPECT(ykhost_preempt_headroom_by_key(h, "ask", 2, NULL) == -1);
  memset(cells, 0x55, sizeof cells);
  EXPECT(ykhost_preempt_headroom_by_key(h, "ask", 0, cells) == YKPRED_E_INVALID && cells[29] == 0 && cells[30] == -1 && cells[0] == 0);
  EXPECT(ykhost_preempt_headroom_by_key(h, "no-such-pod", 2, cells) == YKHOST_E_POD_NOT_FOUND && cells[29] == 2 && cells[30] == -1);
  EXPECT(ykhost_preempt_headroom_by_key(h, "a", 2, cells) == YKHOST_E_NOT_AN_ASK);
  EXPECT(ykhost_preempt_headroom_by_key(h, "ask", 2, cells) == YKPRED_E_STATE);
  EXPECT(ykhost_set_preemption_tiers(h, bounds, 2) == 0);
  EXPECT(ykhost_preempt_headroom(h, 1, &ask0, &two, cells) == YKPRED_E_STATE);      /* tiers or not: a mirror-only handle evaluates nothing */
  ykhost_destroy(h);
  if (failures) return 1;
  printf("preempt headroom ok\n");
  return 0;
}
