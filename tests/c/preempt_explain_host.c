/* preempt_explain_host.c — the host side of preemption explain on a MIRROR-ONLY handle (device -1), for a build of libykhost's sources
 * under AddressSanitizer + UBSan (tests/test_preempt_explain_cpu.py): ykhost_preempt_explain_format on hand-made cells — length query,
 * short buffers, merged texts, the handle's resource names — the limits the mirror derives (ykhost_preempt_limits fails without an
 * engine, ykhost_reclaim_table works), and the errors of the calls that need a device.
 * Exit code 0 and "preempt explain ok" = every call behaved. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ykhost.h"

static int failures = 0;
#define EXPECT(cond)                                                \
  do {                                                              \
    if (!(cond)) {                                                  \
      fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); \
      failures++;                                                   \
    }                                                               \
  } while (0)

static const char* kSnapshot =
    "{\"nodes\":["
    "{\"metadata\":{\"name\":\"n0\"},\"status\":{\"allocatable\":{\"cpu\":\"4\",\"memory\":\"1000\",\"example.com/gpu\":\"2\",\"pods\":\"10\"}},\"pods\":["
    "{\"metadata\":{\"name\":\"a\",\"uid\":\"a\",\"namespace\":\"d\"},\"spec\":{\"priority\":5,\"containers\":[{\"name\":\"c\",\"resources\":{\"requests\":{\"cpu\":\"100m\","
    "\"example.com/gpu\":\"1\"}}}]}}]}],"
    "\"pods\":[{\"metadata\":{\"name\":\"ask\",\"uid\":\"ask\",\"namespace\":\"d\"},\"spec\":{\"priority\":9,\"containers\":[{\"name\":\"c\","
    "\"resources\":{\"requests\":{\"cpu\":\"50m\",\"example.com/gpu\":\"2\"}}}]}}]}";

int main(void) {
  char err[256] = "";
  ykhost_t* h = ykhost_create(-1, err, sizeof err);
  if (!h) {
    fprintf(stderr, "ykhost_create(-1): %s\n", err);
    return 2;
  }
  EXPECT(ykhost_load_snapshot(h, kSnapshot) == 0);
  int64_t cells[32];
  char line[512];
  memset(cells, 0, sizeof cells);
  /* empty total */
  int64_t need = ykhost_preempt_explain_format(h, cells, NULL, 0);
  EXPECT(need == (int64_t)strlen("preemption: 0/0 nodes are available.") + 1);
  EXPECT(ykhost_preempt_explain_format(h, cells, line, sizeof line) == need && strcmp(line, "preemption: 0/0 nodes are available.") == 0);
  EXPECT(ykhost_preempt_explain_format(h, NULL, line, sizeof line) < 0);
  /* every entry, the scalar resource named by the handle, a buffer of every length up to the whole line */
  cells[6] = 14, cells[5] = 3, cells[1] = 2, cells[11] = 1;
  cells[25] = 2, cells[24] = 10, cells[26] = 7, cells[27] = 3, cells[12] = 1, cells[16] = 2, cells[19] = 4;
  need = ykhost_preempt_explain_format(h, cells, NULL, 0);
  EXPECT(need > 1 && need < (int64_t)sizeof line);
  char* whole = (char*)malloc((size_t)need);
  EXPECT(ykhost_preempt_explain_format(h, cells, whole, need) == need && (int64_t)strlen(whole) == need - 1);
  EXPECT(strstr(whole, "preemption: 1/20 nodes are available: ") == whole);
  EXPECT(strstr(whole, "4 Insufficient example.com/gpu") != NULL);
  EXPECT(strstr(whole, "10 No preemption victims found for incoming pod, 2 Insufficient cpu, 2 Preemption is not helpful for scheduling") != NULL);
  for (int64_t len = 1; len < need; ++len) {
    char* part = (char*)malloc((size_t)len); /* exactly len bytes: a write past them is the sanitizer's to find */
    EXPECT(ykhost_preempt_explain_format(h, cells, part, len) == need);
    EXPECT(part[len - 1] == '\0' && strncmp(part, whole, (size_t)len - 1) == 0);
    free(part);
  }
  free(whole);
  /* the limits: the mirror holds the bounds; every call that needs the engine says so */
  int32_t bounds[2] = {6, 9}, limit = -1, dims[4];
  int64_t out[32];
  uint32_t words[1];
  EXPECT(ykhost_preempt_explain(h, 1, NULL, out) < 0);
  EXPECT(ykhost_set_preemption_tiers(h, bounds, 2) == 0);
  EXPECT(ykhost_reclaim_table(h, dims, NULL, NULL, NULL) == 0 && dims[0] == 2 && dims[1] == 4 && dims[3] == 1);
  EXPECT(ykhost_preempt_limits(h, 1, NULL, &limit) < 0 && strstr(ykhost_last_error(h), "mirror-only") != NULL);
  EXPECT(ykhost_preempt_explain(h, 1, NULL, out) < 0 && strstr(ykhost_last_error(h), "mirror-only") != NULL);
  EXPECT(ykhost_preempt_explain_nodes(h, 0, words) < 0 && strstr(ykhost_last_error(h), "mirror-only") != NULL);
  EXPECT(ykhost_preempt_explain_message(h, "ask", line, sizeof line) < 0 && strstr(ykhost_last_error(h), "mirror-only") != NULL);
  EXPECT(ykhost_preempt_explain_message(h, "nobody", line, sizeof line) == YKHOST_E_POD_NOT_FOUND);
  EXPECT(ykhost_preempt_explain_message(h, "a", line, sizeof line) == YKHOST_E_NOT_AN_ASK);
  EXPECT(ykhost_preempt_explain_message(h, NULL, NULL, 0) == YKHOST_E_POD_NOT_FOUND);
  ykhost_destroy(h);
  if (failures) return 1;
  printf("preempt explain ok\n");
  return 0;
}
