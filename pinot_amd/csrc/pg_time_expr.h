// Time-bucket transforms as GROUP BY / DISTINCT keys: the texts ExpressionContext#toString prints for
//   timeconvert(x,'IN','OUT')                                   TimeConversionTransformFunction / JavaTimeUnitTransformer
//   toepoch{seconds,minutes,hours,days}(x), ...rounded(x,'n'), ...bucket(x,'n')      DateTimeFunctions.java:80-268
//   datetimeconvert(x,'inFmt','outFmt','gran')                  EPOCH to EPOCH only (EpochToEpochTransformer)
//   datetrunc('unit',x[,'inUnit'[,'tz'[,'outUnit']]])           DateTruncTransformFunction; tz UTC or a fixed offset +-HH:MM
// parsed into the normal form of pg_time_program.h.  x is ONE plain column (the caller checks its type); every other argument is a literal.
// Every result is LONG.  Plain C++ without HIP types: it compiles stand-alone (tests/time_expr_main.cpp).  Host only.
#pragma once
#include "pg_time_program.h"

#include <string>

namespace pg {
struct TimeProgram {
  std::string column;   // the value argument
  pg_time_program prog;
};
// does the text call a function of the family at its top?  (By canonical name: lower case, underscores dropped.)  Such a text is parsed by
// time_expr_parse; every other expression text by expr_parse (pg_expr.h), which refuses a time function nested inside arithmetic.
bool time_expr_is_time_function(const char* text);
// PG_OK, or PG_ERR_INVALID_ARGUMENT (malformed text, a wrong argument count, an unknown unit name, a malformed format, n = 0, a literal as the
// value argument) / PG_ERR_UNSUPPORTED (a value argument that is no plain column, WEEKS / MONTHS / YEARS units, named time zones, non-epoch
// formats, a bucketing time zone) with the reason in `error`
int32_t time_expr_parse(const char* text, TimeProgram& out, std::string& error);
// the reciprocal of a divisor d != 0 (exposed for the stand-alone test)
pg_time_divisor time_divisor_of(int64_t d);
}  // namespace pg
