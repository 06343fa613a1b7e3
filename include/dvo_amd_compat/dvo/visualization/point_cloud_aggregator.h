// Forwarding header for dvo_core/include/dvo/visualization/point_cloud_aggregator.h: the types live in the MI355X adaptor.
#ifndef DVO_AMD_COMPAT_VISUALIZATION_POINT_CLOUD_AGGREGATOR_H_
#define DVO_AMD_COMPAT_VISUALIZATION_POINT_CLOUD_AGGREGATOR_H_
#include "../../../dvo_amd/point_cloud.hpp"
#endif
