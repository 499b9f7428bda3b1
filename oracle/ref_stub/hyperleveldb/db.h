// TEST SCAFFOLDING ONLY (oracle/Makefile, target _ref/libref_store.so).
// Stand-in for <hyperleveldb/db.h>: empty classes.  DB declares the two
// members daemon/leveldb.h takes the address of; they are defined nowhere and
// never called.
#ifndef hyperleveldb_db_h_
#define hyperleveldb_db_h_
#include <hyperleveldb/slice.h>
#include <hyperleveldb/write_batch.h>
namespace leveldb {
class Snapshot {};
class Iterator {};
class ReplayIterator {};
class Status {};
class DB {
  public:
    void ReleaseSnapshot(const Snapshot* s);
    void ReleaseReplayIterator(ReplayIterator* it);
};
}  // namespace leveldb
#endif
