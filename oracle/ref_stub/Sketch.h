// Stand-in for the sketch library header that the reference's SketchInfo.h includes.  The reference's DBSCAN and
// post-processing sources need it only for five pointer members of SketchInfo and for two MinHash calls inside
// MinHashDBSCAN, a function this project never runs.  Test infrastructure only (oracle/Makefile, target ref).
#ifndef RTC_ORACLE_SKETCH_STUB_H
#define RTC_ORACLE_SKETCH_STUB_H

namespace Sketch {
class MinHash {
 public:
  double distance(MinHash*) { return 1.0; }
  double containDistance(MinHash*) { return 1.0; }
};
class KSSD;
class WMinHash;
class HyperLogLog;
class OrderMinHash;
}  // namespace Sketch

#endif
