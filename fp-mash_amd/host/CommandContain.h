// CommandContain.h — `fpmash contain` (CommandContain.h:16-96): the containment of each query
// in each reference, [score, error-bound, reference-ID, query-ID] per pair.
#pragma once

#include "Command.h"

namespace fpmhost {

class CommandContain : public Command {
public:
    CommandContain();
    int run() const override;
};

}  // namespace fpmhost
