// The model builder's state (ccmi_builder_*): what engine/ingest.cpp fills call by call and ccmi_load_model.cpp appends
// to in bulk (ccmi_builder_populate_from_aggregator). Private to the library; include/ccmi.h only names the struct.
#pragma once
#include <stdint.h>

#include <map>
#include <string>
#include <vector>

namespace ccmi {
namespace ingest {

struct BrokerIn {
  int32_t id;
  int32_t rack;
  double cap[4];
  int32_t state;
  std::string host;  // Rack._hosts key (handleDeadBroker: "UNKNOWN_HOST-<n>", a host of its own)
};
struct DiskIn {
  int32_t brokerId;
  std::string logdir;
  double cap;
  uint8_t demoted = 0;
};

}  // namespace ingest
}  // namespace ccmi

struct ccmi_model_builder {
  int32_t W = 1;
  std::vector<std::string> rackNames;
  std::map<std::string, int32_t> rackIndex;
  std::vector<ccmi::ingest::BrokerIn> brokers;  // creation order
  std::map<int32_t, size_t> brokerById;
  std::vector<ccmi::ingest::DiskIn> disks;
  std::vector<std::string> topics;
  std::map<std::string, int32_t> topicIndex;
  // partitions / replicas in populate order
  std::vector<int32_t> pTopic, pNumber, pOff{0};
  std::vector<int32_t> rBrokerId, rPartition;
  std::vector<uint8_t> rLeader, rOffline;
  std::vector<std::string> rLogdir;  // "" = none
  std::vector<float> rLoad;          // [R][6][W]
  // flattened output (ccmi_builder_desc)
  std::vector<int32_t> oBrokerId, oRack, oState, oRBroker, oPartReplicas, oDiskBroker, oRDisk, oHost;
  std::vector<uint8_t> oDiskDemoted;
  int32_t unknownHosts = 0;
  std::vector<double> oCap, oDiskCap;
  std::vector<const char*> oTopicNames, oDiskLogdir;
  std::vector<int32_t> sortedIds;
};
