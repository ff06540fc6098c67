// How a cell of an OTU table is printed, shared by hmmufotu-amd-sum and the table writer (hu_otu_table.cpp).
#pragma once
#include <sstream>
#include <string>

/* a count as Eigen's IOFormat(FullPrecision) prints a double (src/OTUTable.cpp:26, 161): ostream's general format at precision 15 */
inline std::string hu_num(double v) { std::ostringstream o; o.precision(15); o << v; return o.str(); }
