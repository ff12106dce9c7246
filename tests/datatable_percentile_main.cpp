// A hand-built PERCENTILE result through the host-side DataTable writer (pinot_amd/csrc/pg_datatable.cpp), without a device: compiled and
// run by tests/test_percentile_datatable.py, which checks the bytes it prints (hex) against ObjectSerDeUtils' DoubleArrayList format.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <limits>

#include "pg_internal.hpp"

namespace pg {
void fail(int32_t status, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  fprintf(stderr, "[%d] ", status);
  vfprintf(stderr, fmt, ap);
  fprintf(stderr, "\n");
  va_end(ap);
  exit(2);
}
void DeviceBuffer::release() {}
PinnedBlock::~PinnedBlock() {}
}  // namespace pg

int main() {
  pg::Result r;
  auto alive = std::make_shared<int>(1);
  r.schema_segment = alive;
  r.num_groups = 1;
  r.schema_aggs.resize(2);
  r.schema_aggs[0].name = "*";
  r.schema_aggs[0].function = PG_AGG_COUNT;
  r.schema_aggs[1].name = "lat";
  r.schema_aggs[1].data_type = PG_TYPE_DOUBLE;
  r.schema_aggs[1].function = PG_AGG_PERCENTILE;
  r.aggs.resize(2);
  r.aggs[0].kind = PG_RESULT_LONG;
  r.aggs[0].l[0] = {9};
  pg::AggResult& a = r.aggs[1];
  a.kind = PG_RESULT_VALUE_COUNTS;
  a.param = 99.9;
  a.set_sizes = {5};
  a.d[0] = {-std::numeric_limits<double>::infinity(), -0.0, 0.0, 1.5, std::numeric_limits<double>::quiet_NaN()};
  a.l[0] = {2, 1, 3, 1, 2};
  const std::vector<uint8_t> b = pg::result_data_table_v4(r);
  for (uint8_t x : b) printf("%02x", x);
  printf("\n");
  return 0;
}
