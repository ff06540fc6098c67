// How a cell of an OTU table is printed, shared by hmmufotu-amd-sum and the table writer (hu_otu_table.cpp).
#pragma once
#include <sstream>
#include <string>

/* a count as Eigen's IOFormat(FullPrecision) prints a double (src/OTUTable.cpp:26, 161): ostream's general format at precision 15 */
inline std::string hu_num(double v) { std::ostringstream o; o.precision(15); o << v; return o.str(); }
/* a computed double at 17 significant digits, which name it exactly (hmmufotu-amd-alpha); NaN, a value that does not exist, is "NA" */
inline std::string hu_num17(double v) { if(v != v) return "NA"; std::ostringstream o; o.precision(17); o << v; return o.str(); }
